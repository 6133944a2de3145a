// filter_probe_check.cpp — the resolve step of a launch with per-query predicates, every batch of it under its own table
// (vss_search_multi_filtered_device_begin; a single-table call is a launch of one batch), on a CPU: csrc/filter_groups.h's filter_group_batch_of / filter_group_word_offset
// are the very functions k_resolve_filter_group_batches calls, one thread per launch-wide query.  Here a loop plays the
// threads, over tables and group arrays that are exactly as large as the contract says (so the sanitizers see any read
// outside batch b's n_groups[b] * words words or its n_per_batch group numbers).  A stand-alone program: no HIP, no GPU;
// tests/test_filter_pipeline_host.py builds it again under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../csrc/filter_groups.h"

using namespace vss::host;

#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                               \
			std::exit(1);                                                                                              \
		}                                                                                                              \
	} while (0)

namespace {

// what the kernel writes for query q: the address of its bitmap, or nullptr
const uint64_t *Resolve(const FilterGroupBatch *batches, uint64_t n_per_batch, uint64_t words, uint64_t q) {
	const FilterGroupBatch &d = batches[filter_group_batch_of(n_per_batch, q)];
	const uint64_t at = filter_group_word_offset(d, n_per_batch, words, q);
	return at != NO_GROUP_BITMAP ? d.allowed + at : nullptr;
}

// GraphView::admitted_for's reading of a resolved bitmap
bool Admits(const uint64_t *bitmap, uint64_t n_bits, int64_t key) {
	return bitmap && key >= 0 && (uint64_t)key < n_bits && ((bitmap[(uint64_t)key >> 6] >> ((uint64_t)key & 63)) & 1);
}

// heap arrays of exactly the stated length (a std::vector may keep spare capacity the sanitizer does not guard)
template <class T>
std::unique_ptr<T[]> Exactly(uint64_t n) {
	return std::unique_ptr<T[]>(new T[n]());
}

struct Batch {
	uint64_t n_groups;
	std::unique_ptr<uint64_t[]> table;    // n_groups x words
	std::unique_ptr<uint32_t[]> group_of; // n_per_batch, or none
};

void Launch(uint64_t n_batches, uint64_t n_per_batch, uint64_t n_bits) {
	const uint64_t words = filter_group_words(n_bits);
	std::vector<Batch> batches(n_batches);
	FilterGroupBatch desc[MAX_FILTER_GROUP_BATCHES] = {};
	EXPECT(n_batches <= MAX_FILTER_GROUP_BATCHES);
	for (uint64_t b = 0; b != n_batches; ++b) {
		Batch &x = batches[b];
		x.n_groups = 1 + b % 5;
		EXPECT(filter_group_table_fits(x.n_groups, n_bits));
		x.table = Exactly<uint64_t>(x.n_groups * words);
		// group g of batch b admits the rows whose id is congruent to g + b modulo n_groups + 1 (so the batches differ), and
		// every padding bit after n_bits is SET
		for (uint64_t g = 0; g != x.n_groups; ++g)
			for (uint64_t bit = 0; bit != words * 64; ++bit)
				if (bit >= n_bits || bit % (x.n_groups + 1) == (g + b) % (x.n_groups + 1))
					x.table[g * words + (bit >> 6)] |= uint64_t(1) << (bit & 63);
		if (b % 3 != 2) { // every third batch: NULL group numbers, all its queries take bitmap 0
			x.group_of = Exactly<uint32_t>(n_per_batch);
			for (uint64_t row = 0; row != n_per_batch; ++row)
				x.group_of[row] = (uint32_t)((row + b) % x.n_groups);
			// unknown groups at both edges of the batch: the first past the table, and the largest number there is
			if (b % 2 == 0)
				x.group_of[0] = (uint32_t)x.n_groups;
			else
				x.group_of[n_per_batch - 1] = 0xFFFFFFFFu;
		}
		desc[b] = FilterGroupBatch {x.table.get(), x.group_of.get(), x.n_groups};
	}
	for (uint64_t q = 0; q != n_batches * n_per_batch; ++q) {
		const uint64_t b = q / n_per_batch, row = q % n_per_batch;
		EXPECT(filter_group_batch_of(n_per_batch, q) == b);
		const Batch &x = batches[b];
		const uint64_t *got = Resolve(desc, n_per_batch, words, q);
		const uint64_t group = x.group_of ? x.group_of[row] : 0;
		if (group >= x.n_groups) {
			EXPECT(got == nullptr && !Admits(got, n_bits, 0));
			continue;
		}
		EXPECT(got == x.table.get() + group * words);
		// inside its own table, whole
		EXPECT(got >= x.table.get() && got + words <= x.table.get() + x.n_groups * words);
		for (uint64_t id = 0; id != n_bits + 70; ++id)
			EXPECT(Admits(got, n_bits, (int64_t)id) == (id < n_bits && id % (x.n_groups + 1) == (group + b) % (x.n_groups + 1)));
		EXPECT(!Admits(got, n_bits, -1));
	}
	// the batch edges by name: the last query of batch b - 1 and the first of batch b read different descriptors
	for (uint64_t b = 1; b != n_batches; ++b) {
		EXPECT(filter_group_batch_of(n_per_batch, b * n_per_batch - 1) == b - 1);
		EXPECT(filter_group_batch_of(n_per_batch, b * n_per_batch) == b);
		const uint64_t *last = Resolve(desc, n_per_batch, words, b * n_per_batch - 1);
		const uint64_t *first = Resolve(desc, n_per_batch, words, b * n_per_batch);
		const Batch &p = batches[b - 1], &x = batches[b];
		EXPECT(!last || (last >= p.table.get() && last < p.table.get() + p.n_groups * words));
		EXPECT(!first || (first >= x.table.get() && first < x.table.get() + x.n_groups * words));
	}
}

} // namespace

int main() {
	static_assert(sizeof(FilterGroupBatch) == 24, "32 descriptors by value: 768 bytes of kernel arguments");
	for (uint64_t n_bits : {1ull, 63ull, 64ull, 65ull, 7997ull})
		for (uint64_t n_batches : {1ull, 2ull, 5ull, 32ull})
			for (uint64_t n_per_batch : {1ull, 2ull, 13ull})
				Launch(n_batches, n_per_batch, n_bits);

	// one descriptor, n_per_batch = n_queries: how the single-table calls (vss_search_batch_filtered_groups*) go through the kernel
	const uint32_t groups[6] = {0, 2, 1, 3, 7, 3};
	const uint64_t words = filter_group_words(65);
	auto table = Exactly<uint64_t>(4 * words);
	const FilterGroupBatch one = {table.get(), groups, 4};
	for (uint64_t q = 0; q != 6; ++q) {
		EXPECT(filter_group_batch_of(6, q) == 0);
		EXPECT(filter_group_word_offset(one, 6, words, q) == (groups[q] < 4 ? groups[q] * words : NO_GROUP_BITMAP));
	}
	// tables of different batches may be one address; a NULL group array reads no group number at all
	const FilterGroupBatch same[2] = {{table.get(), nullptr, 1}, {table.get(), nullptr, 4}};
	for (uint64_t q = 0; q != 8; ++q)
		EXPECT(Resolve(same, 4, words, q) == table.get());
	// no bits, no words: every known group resolves to offset 0 and admits nothing
	const FilterGroupBatch empty = {table.get(), groups, 4};
	EXPECT(filter_group_word_offset(empty, 6, 0, 1) == 0 && !Admits(table.get(), 0, 0));
	std::printf("filter probe check ok\n");
	return 0;
}
