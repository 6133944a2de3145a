// label_set_check.cpp — the set half of csrc/label_filter.h on a CPU: the admission rule of a label set, the register form the
// kernels apply to a cell they hold, the padded four-word rows of the walker's table, and the distinct raw rows and group numbers
// of a call.  A stand-alone program (tests/test_label_set_logic.py builds it under the address and undefined-behaviour sanitizers
// and restates every line it prints in NumPy); it also checks the forms against each other and exits non-zero on a difference.
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

// the values whose neighbourhoods decide: both ends of the labels, the sign bit, NO_LABEL and the two below it
static const uint32_t edge[] = {0u, 1u, 2u, 7u, 8u, 9u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
constexpr uint64_t labelled_rows = 11;
constexpr int64_t free_key = 0x7FFFFFFFFFFFFFFFll;

// one set against every edge value as the label, the label in a column of its own so that every key reads it:
// "admit label key result width word ...", keys -1, 0, labelled_rows - 1, labelled_rows, the free key
static void rule_case(const std::vector<uint32_t> &set) {
	const uint32_t width = (uint32_t)set.size(), chunks = label_set_chunks(width);
	std::vector<uint32_t> row(4 * (size_t)chunks); // the walker's table row
	for (uint32_t j = 0; j != 4 * chunks; ++j)
		row[j] = label_set_table_word(set.data(), width, j);
	EXPECT(chunks * 4 >= width && chunks * 4 < width + 4);
	for (uint32_t label : edge) {
		std::vector<uint32_t> column(labelled_rows, label);
		for (int64_t key : {(int64_t)-1, (int64_t)0, (int64_t)labelled_rows - 1, (int64_t)labelled_rows, free_key}) {
			const bool in = label_set_admits(column.data(), labelled_rows, key, set.data(), width);
			std::printf("admit %u %lld %d %u", label, (long long)key, in ? 1 : 0, width);
			for (uint32_t x : set)
				std::printf(" %u", x);
			std::printf("\n");
			if (key >= 0 && (uint64_t)key < labelled_rows) {
				// the walker (GraphView::admitted_set) and the listing kernels get here only with a cell
				EXPECT(in == label_in_set(column[key], set.data(), width));
				EXPECT(in == label_in_padded_set(column[key], row.data(), chunks));
			} else
				EXPECT(!in);
		}
	}
	// a slot without a cell is NO_LABEL in the listing kernels' registers: in no set, whatever its padding
	EXPECT(!label_in_set(NO_LABEL, set.data(), width));
	EXPECT(!label_in_padded_set(NO_LABEL, row.data(), chunks));
}

// "sets width word ..." / "rows word ..." / "group_of ..." triples
static void groups_case(const std::vector<uint32_t> &sets, uint32_t width) {
	const size_t n = sets.size() / width;
	std::vector<uint32_t> rows, group_of, head = {width};
	label_set_groups(sets.data(), n, width, rows, group_of);
	head.insert(head.end(), sets.begin(), sets.end());
	print_list("sets", head);
	print_list("rows", rows);
	print_list("group_of", group_of);
	EXPECT(group_of.size() == n && rows.size() % width == 0);
	for (size_t q = 0; q != n; ++q) {
		EXPECT((size_t)group_of[q] < rows.size() / width);
		for (uint32_t j = 0; j != width; ++j)
			EXPECT(rows[(size_t)group_of[q] * width + j] == sets[q * width + j]);
	}
}

int main() {
	const uint32_t N = NO_LABEL;
	// ---- the rule and both kernel forms: widths 1, 2 and 3 over every combination of the edge values ...
	for (uint32_t a : edge) {
		rule_case({a});
		for (uint32_t b : edge) {
			rule_case({a, b});
			for (uint32_t c : edge)
				rule_case({a, b, c});
		}
	}
	// ... and the widest row: one edge value first, in the middle or LAST among 31 values that are no edge value; every edge value
	// at once; all padding
	for (uint32_t e : edge)
		for (uint32_t at : {0u, 15u, 31u}) {
			std::vector<uint32_t> set(LABEL_SET_MAX);
			for (uint32_t j = 0; j != LABEL_SET_MAX; ++j)
				set[j] = j == at ? e : 100 + j;
			rule_case(set);
		}
	{
		std::vector<uint32_t> set(LABEL_SET_MAX, N);
		rule_case(set);
		for (uint32_t j = 0; j != 11; ++j)
			set[2 * j + 5] = edge[j];
		rule_case(set);
	}
	// a shorter column: the row id has no cell although the array goes on
	{
		const std::vector<uint32_t> column = {5, 5, 5, 5}, set = {4, 5};
		EXPECT(label_set_admits(column.data(), 4, 3, set.data(), 2) && !label_set_admits(column.data(), 3, 3, set.data(), 2));
		EXPECT(!label_set_admits(column.data(), 0, 0, set.data(), 2));
	}
	// width 1 is the call by label, a run of consecutive values the range: label_admits and label_range_admits say the same
	for (uint32_t label : edge)
		for (uint32_t want : edge) {
			EXPECT(label_admits(&label, 1, 0, want) == label_set_admits(&label, 1, 0, &want, 1));
			if (want <= N - 3) {
				const uint32_t run[3] = {want, want + 1, want + 2};
				EXPECT(label_range_admits(&label, 1, 0, want, want + 2) == label_set_admits(&label, 1, 0, run, 3));
			}
		}

	// ---- distinct raw rows and group numbers
	groups_case({3, 9, 3, 9, 3, 9}, 2);                                  // one row
	groups_case({5, 6, 1, 9, 5, 2, 1, 3, 0, N}, 2);                      // all distinct; same first word, different second
	groups_case({4, 8, 9, 2, 4, 8, 7, 1, 9, 2, 4, 8}, 2);                // duplicates
	groups_case({0, 1, N, 1, 0, N, 0, 1, N, N, N, N, 1, 0, N}, 3);       // the same members in two orders: two groups; all padding
	groups_case({N, N, 2, N, N, N, N, 2}, 2);                            // all padding at another width; padding ahead of a value
	groups_case({0x80000000u, 1, 0x7FFFFFFFu, 2, 0, 0x80000000u, 0, 0x7FFFFFFFu}, 2); // ordered as unsigned words
	groups_case({7, 3, 7, 2, 7}, 1);                                     // width 1
	groups_case({}, 2);                                                  // no queries
	{
		uint64_t s = 0x9E3779B97F4A7C15ull;
		auto rnd = [&]() {
			s ^= s << 13, s ^= s >> 7, s ^= s << 17;
			return (uint32_t)(s >> 32);
		};
		std::vector<uint32_t> sets(300 * 4);
		for (uint32_t &x : sets)
			x = rnd() % 3 ? rnd() % 3 : N;
		groups_case(sets, 4);
		std::vector<uint32_t> wide(40 * LABEL_SET_MAX);
		for (uint32_t &x : wide)
			x = rnd() % 2;
		for (size_t j = 0; j != LABEL_SET_MAX; ++j) // rows that differ in the last word only
			wide[j] = wide[LABEL_SET_MAX + j] = 1;
		wide[LABEL_SET_MAX - 1] = 0;
		groups_case(wide, LABEL_SET_MAX);
	}

	if (failures) {
		std::printf("label set check FAILED: %d\n", failures);
		return 1;
	}
	std::printf("label set check ok\n");
	return 0;
}
