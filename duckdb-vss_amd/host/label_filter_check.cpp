// label_filter_check.cpp — csrc/label_filter.h on a CPU: the distinct values and group numbers of a `want` array, the lookup the
// label listing kernels run, the admission rule, the validation of vss_set_labels' range and its gap filling.  A stand-alone
// program (tests/test_label_filter_logic.py builds it under the address and undefined-behaviour sanitizers and restates every
// line it prints in NumPy); it also checks itself against naive restatements and exits non-zero on a difference.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
	rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 32);
}

static void print_list(const char *tag, const std::vector<uint32_t> &v) {
	std::printf("%s", tag);
	for (uint32_t x : v)
		std::printf(" %u", x);
	std::printf("\n");
}

// "want ..." / "values ..." / "group_of ..." triples
static void groups_case(const std::vector<uint32_t> &want) {
	std::vector<uint32_t> values, group_of;
	label_groups(want.data(), want.size(), values, group_of);
	print_list("want", want);
	print_list("values", values);
	print_list("group_of", group_of);
	EXPECT(group_of.size() == want.size());
	for (size_t i = 1; i < values.size(); ++i)
		EXPECT(values[i - 1] < values[i]);
	for (size_t q = 0; q != want.size(); ++q) {
		EXPECT(group_of[q] < values.size() && values[group_of[q]] == want[q]);
		// the lookup finds every wanted value but NO_LABEL where the kernels look it up
		const uint32_t g = label_lookup(values.data(), (uint32_t)values.size(), want[q]);
		EXPECT(g == (want[q] == NO_LABEL ? NO_LABEL_GROUP : group_of[q]));
	}
}

// "lookupset U v..." then "lookup U label result" lines: every value, its neighbours, both ends, NO_LABEL
static void lookup_case(uint32_t U, bool with_no_label, bool dense) {
	std::vector<uint32_t> values(U);
	uint32_t v = dense ? 0 : rnd() % 5;
	for (uint32_t i = 0; i != U; ++i) {
		values[i] = v;
		v += dense ? 1 : 1 + rnd() % 7;
	}
	if (with_no_label)
		values[U - 1] = NO_LABEL;
	if (!dense && U > 1 && !with_no_label)
		values[U - 1] = 0xFFFFFFFEu; // 2^32 - 2: the largest label
	std::printf("lookupset %u", U);
	for (uint32_t x : values)
		std::printf(" %u", x);
	std::printf("\n");
	std::vector<uint32_t> probes = {0u, 1u, 0xFFFFFFFEu, NO_LABEL};
	for (uint32_t x : values) {
		probes.push_back(x);
		probes.push_back(x + 1u);
		probes.push_back(x - 1u);
	}
	for (uint32_t label : probes) {
		const uint32_t got = label_lookup(values.data(), U, label);
		uint32_t naive = NO_LABEL_GROUP;
		for (uint32_t i = 0; i != U; ++i)
			if (values[i] == label && label != NO_LABEL)
				naive = i;
		EXPECT(got == naive);
		std::printf("lookup %u %u %u\n", U, label, got);
	}
}

int main() {
	// ---- distinct values and group numbers
	groups_case({7, 7, 7, 7, 7});                                   // all equal
	groups_case({9, 3, 5, 1, 8, 2});                                // all distinct
	groups_case({NO_LABEL, 4, NO_LABEL, 4, 0});                     // a NULL tenant: the last group
	groups_case({0, 0xFFFFFFFEu, 0, 0xFFFFFFFEu, NO_LABEL, 17});    // both ends of the label range
	groups_case({NO_LABEL});
	groups_case({});
	{
		std::vector<uint32_t> want(300);
		for (uint32_t &w : want)
			w = rnd() % 40 == 0 ? NO_LABEL : rnd() % 97;
		groups_case(want);
	}

	// ---- the lookup of the listing kernels
	for (uint32_t U : {1u, 2u, 63u, 64u, 65u, 1024u}) {
		lookup_case(U, false, false);
		lookup_case(U, true, false);
		lookup_case(U, false, true);
	}
	EXPECT(label_lookup(nullptr, 0, 5) == NO_LABEL_GROUP); // no values: nothing is read

	// ---- the wanted value as the walker compares it
	for (uint32_t want : {0u, 1u, 0xFFFFFFFEu, NO_LABEL}) {
		std::printf("cell %u %llu\n", want, (unsigned long long)label_want_cell(want));
		for (uint32_t label : {0u, 1u, 0xFFFFFFFEu, NO_LABEL})
			EXPECT(((uint64_t)label == label_want_cell(want)) == (label == want && want != NO_LABEL));
	}

	// ---- admission: "admit labelled_rows key want result" over the column "labels ..."
	{
		const std::vector<uint32_t> labels = {5, NO_LABEL, 0, 5, 0xFFFFFFFEu, 7, 5, NO_LABEL};
		print_list("labels", labels);
		for (uint64_t labelled : {(uint64_t)labels.size(), (uint64_t)4, (uint64_t)0})
			for (int64_t key : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)4, (int64_t)6, (int64_t)7, (int64_t)8, (int64_t)1 << 40})
				for (uint32_t want : {5u, 0u, 0xFFFFFFFEu, NO_LABEL, 9u}) {
					const bool in = label_admits(labels.data(), labelled, key, want);
					std::printf("admit %llu %lld %u %d\n", (unsigned long long)labelled, (long long)key, want, in ? 1 : 0);
					// ... and the walker's one comparison says the same wherever the row has a cell
					if (key >= 0 && (uint64_t)key < labelled)
						EXPECT(in == ((uint64_t)labels[key] == label_want_cell(want)));
					else
						EXPECT(!in);
				}
	}

	// ---- the range of vss_set_labels: "range first n fault" (0 none, 1 no labels, 2 too far)
	{
		const uint32_t cell = 0;
		const uint64_t two32 = 1ull << 32;
		struct Case {
			const void *p;
			uint64_t first, n;
		};
		const Case cases[] = {{&cell, 0, 1}, {&cell, two32 - 1, 1}, {&cell, two32 - 1, 2}, {&cell, two32, 0}, {&cell, two32, 1},
		                      {&cell, 0, two32}, {&cell, 0, two32 + 1}, {&cell, 1, two32}, {&cell, two32 - 100, 100}, {&cell, two32 - 100, 101},
		                      {nullptr, 0, 0}, {nullptr, 0, 1}, {nullptr, two32 + 5, 0}, {&cell, ~0ull, 2}, {&cell, 5, ~0ull},
		                      {&cell, two32 + 1, 1}, {&cell, ~0ull, ~0ull}};
		for (const Case &c : cases) {
			const LabelRangeFault f = check_label_range(c.p, c.first, c.n);
			std::printf("range %d %llu %llu %d\n", c.p ? 1 : 0, (unsigned long long)c.first, (unsigned long long)c.n, (int)f);
		}
	}

	// ---- growth and gap filling: "write labelled first n rows_after gap_begin gap_end", and a column carried along
	{
		std::vector<uint32_t> column, model; // `model`: the naive restatement, resized and filled cell by cell
		struct W {
			uint64_t first, n;
		};
		const W writes[] = {{0, 4}, {4, 3}, {10, 2}, {2, 3}, {11, 5}, {30, 1}, {0, 31}, {31, 1}, {40, 1}, {5, 1}};
		uint32_t next = 100;
		for (const W &wr : writes) {
			const LabelWrite w = label_write(column.size(), wr.first, wr.n);
			std::printf("write %llu %llu %llu %llu %llu %llu\n", (unsigned long long)column.size(), (unsigned long long)wr.first,
			            (unsigned long long)wr.n, (unsigned long long)w.rows_after, (unsigned long long)w.gap_begin,
			            (unsigned long long)w.gap_end);
			EXPECT(w.gap_begin <= w.gap_end && w.gap_end <= w.rows_after);
			// as the engine does: grow, fill the gap, write
			column.resize(w.rows_after, 0xDEADBEEFu); // (fresh device memory holds anything)
			for (uint64_t r = w.gap_begin; r != w.gap_end; ++r)
				column[r] = NO_LABEL;
			if (model.size() < wr.first + wr.n)
				model.resize(wr.first + wr.n, NO_LABEL);
			for (uint64_t i = 0; i != wr.n; ++i)
				column[wr.first + i] = model[wr.first + i] = next++;
			EXPECT(column == model);
		}
	}

	if (failures) {
		std::printf("label filter check FAILED: %d\n", failures);
		return 1;
	}
	std::printf("label filter check ok\n");
	return 0;
}
