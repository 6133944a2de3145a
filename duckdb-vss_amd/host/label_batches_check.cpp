// label_batches_check.cpp — the "several batches" part of csrc/label_filter.h on a CPU: the walk table of a launch by label whose
// batches each bring their own device matrices (vss_search_by_label_device_begin, vss_search_multi_by_label_device_begin), written
// unit by unit as k_resolve_label_batches / k_resolve_label_batches64 write it, against the table the six single-batch resolve
// kernels make of the same queries laid end to end — cell for cell, head included, for every kind.  Every batch's matrices are heap
// blocks of exactly their size, so a unit that reads beyond its batch is caught.  A stand-alone program
// (tests/test_label_batches_logic.py builds it under the address and undefined-behaviour sanitizers and checks its count of cases);
// it exits non-zero on a difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../csrc/label_filter.h"

using namespace vss::host;

static int failures = 0;
static unsigned long long table_cases = 0, map_cases = 0;
#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			if (failures < 20)                                                                                         \
				std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                          \
			++failures;                                                                                                \
		}                                                                                                              \
	} while (0)

constexpr uint64_t UNWRITTEN = 0xA5A5A5A5A5A5A5A5ull;
constexpr uint64_t ADDRESSES[LABEL_COLUMNS_MAX] = {0x7F0000001000ull, 0x7F0000002000ull, 0x7F0000003000ull, 0x7F0000004000ull};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
	rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
	return rng_state;
}
// a word of a predicate: the edges of its width among values that leave room for lo <= hi and lo > hi alike
template <class W>
static W word() {
	constexpr W none = (W)~(W)0;
	const W edge[] = {0, 1, (W)(none - 1), none, (W)((W)1 << (8 * sizeof(W) - 1)), (W)0xFFFFFFFFull, (W)0x100000000ull};
	const uint64_t r = rng();
	return r % 3 == 0 ? edge[(r >> 8) % 7] : (W)((r >> 8) % 1000);
}

// the words of one launch: per batch three heap blocks of exactly the batch's size, and the same words laid end to end
template <class W>
struct Launch {
	uint64_t n_batches, per_batch;
	std::vector<std::unique_ptr<W[]>> blocks;
	std::vector<LabelBatch<W>> batches;
	std::vector<W> words, lo, hi; // launch-wide: batch after batch
	Launch(uint64_t nb, uint64_t pb, uint64_t words_per_query, uint64_t ends_per_query) : n_batches(nb), per_batch(pb) {
		for (uint64_t b = 0; b != nb; ++b) {
			W *block[3] = {};
			const uint64_t n[3] = {pb * words_per_query, pb * ends_per_query, pb * ends_per_query};
			std::vector<W> *all[3] = {&words, &lo, &hi};
			for (int part = 0; part != 3; ++part) {
				if (!n[part])
					continue; // (what a kind does not use stays a null pointer: reading it would fault)
				blocks.emplace_back(new W[n[part]]);
				block[part] = blocks.back().get();
				for (uint64_t i = 0; i != n[part]; ++i)
					all[part]->push_back(block[part][i] = word<W>());
			}
			batches.push_back({block[0], block[1], block[2]});
		}
	}
};

// the launch's table as the resolve kernels write it: a grid of 256-thread blocks, thread i the head cell i and unit i
template <class W>
static std::vector<uint64_t> batched_table(const Launch<W> &launch, const LabelBatchShape &s, uint32_t wide_mask) {
	const uint64_t nq = launch.n_batches * launch.per_batch, units = nq * label_batches_query_units(s);
	std::vector<uint64_t> table(label_batches_table_cells(s, nq), UNWRITTEN);
	const LabelTableHead head = label_batches_table_head(s, ADDRESSES, wide_mask);
	EXPECT(head.n == label_batches_query_base(s) && head.n <= LABEL_TABLE_HEAD_MAX);
	for (uint64_t i = 0; i != (units / 256 + 1) * 256; ++i) {
		if (i < head.n)
			table[i] = head.cell[i];
		if (i >= units)
			continue;
		if constexpr (sizeof(W) == 8) {
			table.at(head.n + i) = label_batches_cell64(launch.batches.data(), s, i);
		} else if (s.kind == LabelKind::SET) {
			EXPECT(head.n + i / 2 < table.size());
			const uint32_t w = label_batches_set_word(launch.batches.data(), s, i);
			std::memcpy(reinterpret_cast<unsigned char *>(table.data() + head.n) + 4 * i, &w, 4);
		} else {
			table.at(head.n + i) = label_batches_cell(launch.batches.data(), s, i);
		}
	}
	return table;
}

static void compare(const std::vector<uint64_t> &got, const std::vector<uint64_t> &want) {
	++table_cases;
	EXPECT(got.size() == want.size());
	EXPECT(got == want);
	for (const uint64_t cell : want)
		if (cell == UNWRITTEN) {
			EXPECT(!"a cell of the single-batch table was never written");
			break;
		}
}

// ---- the six single-batch tables over the launch-wide matrices: the bodies of k_resolve_label_wants .. k_resolve_label_set_boxes
static std::vector<uint64_t> single_eq(const std::vector<uint32_t> &want) {
	std::vector<uint64_t> t(1 + want.size(), UNWRITTEN);
	t[0] = ADDRESSES[0];
	for (size_t q = 0; q != want.size(); ++q)
		t[1 + q] = label_want_cell(want[q]);
	return t;
}
static std::vector<uint64_t> single_range(const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi) {
	std::vector<uint64_t> t(1 + 2 * lo.size(), UNWRITTEN);
	t[0] = ADDRESSES[0];
	for (size_t q = 0; q != lo.size(); ++q) {
		const LabelRangeCells c = label_range_cells(lo[q], hi[q]);
		t[1 + 2 * q] = c.lo, t[2 + 2 * q] = c.width;
	}
	return t;
}
static std::vector<uint64_t> single_set(const std::vector<uint32_t> &sets, uint32_t width, uint64_t nq) {
	const uint32_t padded = 4 * label_set_chunks(width);
	std::vector<uint64_t> t(2 + 2 * (uint64_t)label_set_chunks(width) * nq, UNWRITTEN);
	t[0] = ADDRESSES[0], t[1] = width;
	for (uint64_t i = 0; i != nq * padded; ++i) {
		const uint64_t q = i / padded;
		const uint32_t w = label_set_table_word(sets.data() + q * width, width, (uint32_t)(i - q * padded));
		std::memcpy(reinterpret_cast<unsigned char *>(t.data() + 2) + 4 * i, &w, 4);
	}
	return t;
}
static std::vector<uint64_t> single_box(const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi, uint32_t m, uint64_t nq) {
	std::vector<uint32_t> boxes;
	label_box_rows(lo.data(), hi.data(), nq, m, boxes);
	std::vector<uint64_t> t(label_box_table_cells(m, nq), UNWRITTEN);
	t[0] = m;
	for (uint32_t j = 0; j != m; ++j)
		t[1 + j] = ADDRESSES[j];
	for (uint64_t i = 0; i != nq * m; ++i) {
		const LabelRangeCells c = label_range_cells(boxes[2 * i], boxes[2 * i + 1]);
		t[1 + m + 2 * i] = c.lo, t[2 + m + 2 * i] = c.width;
	}
	return t;
}
static std::vector<uint64_t> single_box64(const std::vector<uint64_t> &lo, const std::vector<uint64_t> &hi, uint32_t m, uint64_t nq,
                                          uint32_t wide_mask) {
	std::vector<uint32_t> boxes;
	label_box64_rows(lo.data(), hi.data(), nq, m, boxes);
	std::vector<uint64_t> t(label_box_table_cells(m, nq), UNWRITTEN);
	t[0] = label_box64_table_head(m, wide_mask);
	for (uint32_t j = 0; j != m; ++j)
		t[1 + j] = ADDRESSES[j];
	for (uint64_t i = 0; i != nq * m; ++i) {
		const LabelRange64Cells c =
		    label_range64_cells(label_word64(boxes[4 * i], boxes[4 * i + 1]), label_word64(boxes[4 * i + 2], boxes[4 * i + 3]));
		t[1 + m + 2 * i] = c.lo, t[2 + m + 2 * i] = c.count;
	}
	return t;
}
static std::vector<uint64_t> single_set_box(const std::vector<uint64_t> &sets, uint32_t width, const std::vector<uint64_t> &lo,
                                            const std::vector<uint64_t> &hi, uint32_t m, uint64_t nq, uint32_t wide_mask) {
	std::vector<uint32_t> rows;
	label_set_box_rows(sets.data(), width, lo.data(), hi.data(), nq, m, rows);
	const uint32_t padded = label_set_box_padded(width), per = (uint32_t)label_set_box_query_cells(m, padded);
	std::vector<uint64_t> t(label_set_box_table_cells(m, padded, nq), UNWRITTEN);
	t[0] = label_set_box_table_head(m, padded, wide_mask);
	for (uint32_t j = 0; j <= m; ++j)
		t[1 + j] = ADDRESSES[j];
	if (2 + m < label_set_box_query_base(m))
		t[2 + m] = 0;
	for (uint64_t i = 0; i != nq * per; ++i)
		t[label_set_box_query_base(m) + i] =
		    label_set_box_table_cell(rows.data() + (i / per) * label_set_box_row_words(width, m), width, m, (uint32_t)(i % per));
	return t;
}

// where the launch puts query q's share is where the form's own table puts query q
static void offsets(const LabelBatchShape &s, uint64_t nq) {
	const uint64_t units = label_batches_query_units(s), base = label_batches_query_base(s);
	for (uint64_t q : {uint64_t(0), nq / 2, nq - 1, nq}) {
		++map_cases;
		const uint64_t at = base + (s.kind == LabelKind::SET ? units / 2 : units) * q;
		if (s.kind == LabelKind::EQ)
			EXPECT(at == 1 + q);
		else if (s.kind == LabelKind::RANGE)
			EXPECT(at == 1 + 2 * q);
		else if (s.kind == LabelKind::SET)
			EXPECT(at == 2 + 2 * (uint64_t)label_set_chunks(s.width) * q);
		else if (s.kind == LabelKind::SET_BOX)
			EXPECT(at == label_set_box_query_cell(s.m, label_set_box_padded(s.width), q));
		else
			EXPECT(at == label_box_query_cell(s.m, q));
	}
}

int main() {
	const uint64_t per_batches[] = {1, 2, 13, 256}, batch_counts[] = {1, 5, 32};
	const uint32_t widths[] = {1, 4, 5, 32};
	static_assert(LABEL_BATCHES_MAX == 32, "the largest launch of the cases below");
	for (const uint64_t pb : per_batches)
		for (const uint64_t nb : batch_counts) {
			const uint64_t nq = nb * pb;
			// launch-wide query -> (batch, row), at the seams of every batch
			for (uint64_t b = 0; b != nb; ++b)
				for (const uint64_t row : {uint64_t(0), pb / 2, pb - 1}) {
					++map_cases;
					const LabelBatchAt at = label_batch_at(pb, b * pb + row);
					EXPECT(at.batch == b && at.row == row);
				}
			{
				const LabelBatchShape s = {LabelKind::EQ, 0, 0, (uint32_t)pb};
				const Launch<uint32_t> l(nb, pb, 1, 0);
				compare(batched_table(l, s, 0), single_eq(l.words));
				offsets(s, nq);
			}
			{
				const LabelBatchShape s = {LabelKind::RANGE, 0, 0, (uint32_t)pb};
				const Launch<uint32_t> l(nb, pb, 0, 1);
				compare(batched_table(l, s, 0), single_range(l.lo, l.hi));
				offsets(s, nq);
			}
			for (const uint32_t width : widths) {
				const LabelBatchShape s = {LabelKind::SET, width, 0, (uint32_t)pb};
				const Launch<uint32_t> l(nb, pb, width, 0);
				compare(batched_table(l, s, 0), single_set(l.words, width, nq));
				offsets(s, nq);
			}
			for (uint32_t m = 1; m <= LABEL_COLUMNS_MAX; ++m) {
				const LabelBatchShape s = {LabelKind::BOX, 0, m, (uint32_t)pb};
				const Launch<uint32_t> l(nb, pb, 0, m);
				compare(batched_table(l, s, 0), single_box(l.lo, l.hi, m, nq));
				offsets(s, nq);
				const LabelBatchShape s64 = {LabelKind::BOX64, 0, m, (uint32_t)pb};
				const uint32_t wide_mask = (uint32_t)(rng() & ((1u << m) - 1));
				const Launch<uint64_t> l64(nb, pb, 0, m);
				compare(batched_table(l64, s64, wide_mask), single_box64(l64.lo, l64.hi, m, nq, wide_mask));
				offsets(s64, nq);
			}
			for (const uint32_t width : widths)
				for (uint32_t m = 0; m <= LABEL_SET_BOX_RANGES_MAX; ++m) {
					const LabelBatchShape s = {LabelKind::SET_BOX, width, m, (uint32_t)pb};
					const uint32_t wide_mask = (uint32_t)(rng() & ((2u << m) - 1));
					const Launch<uint64_t> l(nb, pb, width, m);
					compare(batched_table(l, s, wide_mask), single_set_box(l.words, width, l.lo, l.hi, m, nq, wide_mask));
					offsets(s, nq);
				}
		}
	std::printf("table cases %llu\n", table_cases);
	std::printf("map cases %llu\n", map_cases);
	if (failures) {
		std::printf("%d FAILED\n", failures);
		return 1;
	}
	std::printf("label batches check ok\n");
	return 0;
}
