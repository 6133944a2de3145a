// vss_engine.hip — host side of libvssgpu.so: device memory management, the batch-synchronous build schedule,
// kernel launches, the usearch-compatible stream format, and the C ABI declared in include/vssgpu.h.
//
// What it replaces in the reference: the `unum::usearch::index_dense_gt<row_t> index` member of HNSWIndex
// (reference src/include/hnsw/hnsw_index.hpp:45) — i.e. index_dense.hpp + index.hpp + index_plugins.hpp of the
// vendored usearch.  Nothing here depends on oracle/ (test infrastructure); without a HIP device every entry
// point fails loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#define VSS_ENGINE_TU
#include "../../include/vssgpu.h"
#include "launchers.h"
#include "host_logic.h"
#include "filter_groups.h"
#include "label_filter.h"
#include "exact_filtered_kernels.h"
#include "filter_route_kernels.h"
#include "row_codes.h"

using namespace vss;
using namespace vss::host;

// the one rule host_logic.h still restates for the CPU tests (team_touch_lines_max) is the kernels'
static_assert(team_touch_max_lines(0) == 8 && team_touch_max_lines(1) == 8 && team_touch_max_lines(3) == 24, "helper touch window");

namespace {

// ---------------------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------------------
struct HipError {
	hipError_t code;
	const char *what;
};

#define HIP_TRY(expr)                                                                                                  \
	do {                                                                                                               \
		hipError_t _e = (expr);                                                                                        \
		if (_e != hipSuccess)                                                                                          \
			throw HipError {_e, #expr};                                                                                \
	} while (0)

template <typename T>
struct DevBuf {
	T *p = nullptr;
	size_t n = 0;
	void free() {
		if (p)
			(void)hipFree(p);
		p = nullptr;
		n = 0;
	}
	// grow to at least `want` elements, preserving the first `keep` elements
	void ensure(size_t want, size_t keep, hipStream_t s, int fill_byte = -1) {
		if (want <= n)
			return;
		T *np = nullptr;
		HIP_TRY(hipMalloc(&np, want * sizeof(T)));
		if (fill_byte >= 0)
			HIP_TRY(hipMemsetAsync(np, fill_byte, want * sizeof(T), s));
		if (p && keep)
			HIP_TRY(hipMemcpyAsync(np, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (p)
			(void)hipFree(p);
		p = np;
		n = want;
	}
	// grow to at least `want` elements, contents undefined; false (nothing changed but a freed buffer) when the device has no room.
	// Frees FIRST: for the large optional buffers (row codes, retry tables) whose old and new sizes may not fit side by side and
	// whose loss only turns an optimisation off.  A buffer a call cannot do without takes try_grow.
	bool try_ensure(size_t want) {
		if (want <= n)
			return true;
		free();
		T *np = nullptr;
		if (hipMalloc(&np, want * sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();
			return false;
		}
		p = np;
		n = want;
		return true;
	}
	// the same, but the new buffer is allocated BEFORE the old one is freed (the order ADVICE.md asks for): on failure the buffer
	// stays exactly as it was and the call that needed it fails alone.  For the small per-call tables of the search contexts.
	bool try_grow(size_t want) {
		if (want <= n)
			return true;
		T *np = nullptr;
		if (hipMalloc(&np, want * sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();
			return false;
		}
		if (p)
			(void)hipFree(p);
		p = np;
		n = want;
		return true;
	}
};

} // namespace

// ---------------------------------------------------------------------------------------------------------
// the index
// ---------------------------------------------------------------------------------------------------------
// result.error.what() of the calling thread's last failed call (searches run concurrently: one string per thread)
static thread_local std::string tls_error;

// What a search launch filters its results by.  The pointers are device memory for search_begin / search_launch and host
// memory for search_host, which stages what they name and hands search_launch the staged copy.
struct SearchPredicate {
	enum Kind { NONE, ONE_BITMAP, PER_QUERY, BY_LABEL, BY_RANGE, BY_SET, BY_BOX, BY_BOX64, BY_SET_BOX } kind = NONE;
	const uint64_t *bitmap = nullptr;                        // ONE_BITMAP: the whole launch's; bit set = row id admitted
	FilterGroupBatch batches[MAX_FILTER_GROUP_BATCHES] = {}; // PER_QUERY: the table of every batch of the launch
	uint64_t n_bits = 0;                                     // (BY_LABEL: the cells of the index's label column)
	const uint32_t *want = nullptr;                          // BY_LABEL: the label every query of the (one) batch wants
	const uint32_t *lo = nullptr, *hi = nullptr;             // BY_RANGE: the ends of every query's label range, both inclusive
	const uint32_t *sets = nullptr;                          // BY_SET: `width` words per query, row-major
	uint32_t width = 0;
	const uint32_t *boxes = nullptr;                         // BY_BOX: 2 * n_columns words per query, (lo, hi) per named column
	                                                         // BY_BOX64: 4 * n_columns words per query (label_box64_rows)
	                                                         // BY_SET_BOX: the travelling rows (label_set_box_rows); `width` is the
	                                                         // set's, columns[0] the set column, columns[1 ..] the range columns
	uint32_t n_columns = 0, columns[LABEL_COLUMNS_MAX] = {}; // BY_BOX: the label columns the call names (n_bits: the shortest one's cells)
	// The BY_ kinds of the _begin calls: every batch of the launch brings its own words, SEPARATE device matrices as the form's
	// _device call takes them (label_filter.h, "several batches"), and want / lo / hi / sets / boxes above stay null.
	bool by_batches = false;
	struct LabelWords {
		const void *words, *lo, *hi; // words: BY_LABEL's want, BY_SET's and BY_SET_BOX's sets
	} label_words[MAX_FILTER_GROUP_BATCHES] = {};
	// this BY_ predicate over `words`, one entry per batch of the launch
	SearchPredicate with_batches(const LabelWords (&words)[MAX_FILTER_GROUP_BATCHES]) const {
		SearchPredicate p = *this;
		p.by_batches = true;
		std::copy(words, words + MAX_FILTER_GROUP_BATCHES, p.label_words);
		return p;
	}

	// a launch of one batch against the index's label column: query q admits the rows labelled want[q]
	static SearchPredicate by_label(const uint32_t *want, uint64_t labelled_rows) {
		SearchPredicate p;
		p.kind = BY_LABEL, p.n_bits = labelled_rows, p.want = want;
		return p;
	}

	// ... query q admits the rows whose label lies in [lo[q], hi[q]]
	static SearchPredicate by_range(const uint32_t *lo, const uint32_t *hi, uint64_t labelled_rows) {
		SearchPredicate p;
		p.kind = BY_RANGE, p.n_bits = labelled_rows, p.lo = lo, p.hi = hi;
		return p;
	}

	// ... query q admits the rows whose label is one of sets[q * width .. (q + 1) * width)
	static SearchPredicate by_set(const uint32_t *sets, uint32_t width, uint64_t labelled_rows) {
		SearchPredicate p;
		p.kind = BY_SET, p.n_bits = labelled_rows, p.sets = sets, p.width = width;
		return p;
	}

	// ... query q admits the rows whose cell in named column j lies in [boxes[2 m q + 2 j], boxes[2 m q + 2 j + 1]] for every j < m
	static SearchPredicate by_box(const uint32_t *boxes, const uint32_t *columns, uint32_t m, uint64_t shortest_rows) {
		SearchPredicate p;
		p.kind = BY_BOX, p.n_bits = shortest_rows, p.boxes = boxes, p.n_columns = m;
		std::copy(columns, columns + m, p.columns);
		return p;
	}

	// ... the same with 64-bit ends: 4m words per query, per named column lo then hi, each as (high word, low word)
	static SearchPredicate by_box64(const uint32_t *boxes, const uint32_t *columns, uint32_t m, uint64_t shortest_rows) {
		SearchPredicate p = by_box(boxes, columns, m, shortest_rows);
		p.kind = BY_BOX64;
		return p;
	}

	// ... query q admits what row q of `rows` (2 width + 4 (n - 1) words, label_set_box_rows) admits: columns[0] is the set column,
	// columns[1 .. n) the range columns
	static SearchPredicate by_set_box(const uint32_t *rows, uint32_t width, const uint32_t *columns, uint32_t n, uint64_t shortest_rows) {
		SearchPredicate p = by_box(rows, columns, n, shortest_rows);
		p.kind = BY_SET_BOX, p.width = width;
		return p;
	}

	static SearchPredicate one_bitmap(const uint64_t *bitmap, uint64_t n_bits) {
		return {ONE_BITMAP, bitmap, {}, n_bits};
	}
	// a launch of one batch under one table: query q takes bitmap group_of[q]
	static SearchPredicate one_table(const uint64_t *allowed, const uint32_t *group_of, uint64_t n_groups, uint64_t n_bits) {
		return {PER_QUERY, nullptr, {{allowed, group_of, n_groups}}, n_bits};
	}
};
static_assert((uint32_t)MAX_COALESCED == MAX_FILTER_GROUP_BATCHES, "one descriptor per batch of a launch");

// One launch of the search engine: n_batches probe batches of per_batch queries each, batch b read from queries[b] and answered
// into out_keys[b] / out_d[b] (may be NULL) / out_count[b].  vss_index::request fills everything but the named options.
struct SearchRequest {
	int slot = 0; // the context that carries the launch
	uint64_t n_batches = 1, per_batch = 0;
	const float *const *queries = nullptr;
	int64_t *const *out_keys = nullptr;
	float *const *out_d = nullptr;
	uint32_t *const *out_count = nullptr;
	uint32_t q_stride = 0;
	uint64_t k = 0, ef = 0;
	SearchPredicate predicate;
	bool direct_io = false;        // queries and answers live in pinned host memory (the small-batch probe)
	bool gate = false;             // issue the launch when the previous one starts to drain (the pipelined calls)
	bool keep_query_stats = false; // search_launch: keep every query's counters for vss_last_query_stats
};

// ---- the scan side's counterpart of the two values above (the exact scan under predicates, the routed call, the calls by label)
// A per-query column of 32-bit words, marked by the memory it lives in: the plans read such a column on the host, the walk on the
// device, and both are `const uint32_t *`.
struct HostWords {
	const uint32_t *p;
	explicit HostWords(const uint32_t *host) : p(host) {
	}
};
struct DeviceWords {
	const uint32_t *p;
	explicit DeviceWords(const uint32_t *device) : p(device) {
	}
};
// The label columns a call by label box names, in call order, as the index holds them while the call runs (under its lock): their
// numbers, their DEVICE cells, how many cells each has and how wide a cell is (32 or 64 bits; a 64-bit cell is two words of `cells`).
struct LabelBoxColumns {
	uint32_t m = 0, columns[LABEL_COLUMNS_MAX] = {};
	const uint32_t *cells[LABEL_COLUMNS_MAX] = {};
	uint64_t rows[LABEL_COLUMNS_MAX] = {};
	uint32_t width[LABEL_COLUMNS_MAX] = {};
	uint32_t wide_mask() const { // bit j: named column j is 64 bits wide
		uint32_t mask = 0;
		for (uint32_t j = 0; j != m; ++j)
			mask |= (uint32_t)(width[j] == 64) << j;
		return mask;
	}
	uint64_t shortest_rows() const {
		return *std::min_element(rows, rows + m);
	}
};

// The groups the rows of a scan call are listed by, made by one of the seven factories only.  Bitmaps: group g = the rows bitmap g
// of a DEVICE table admits.  Labels: group g = the rows the index's label column gives values[g], the ascending distinct wanted
// values (HOST memory); no bitmap exists.  Either way query q reads group group_of[q] (HOST memory; nullptr: all read group 0),
// and the walk of the graph-routed queries reads the column's DEVICE twin: group numbers under bitmaps, wanted labels under labels.
// Ranges: group g = the rows whose label lies within pairs[g], the ascending distinct raw (lo, hi) pairs of the call (HOST memory);
// the walk reads TWO device columns, every query's lo (d_group_of) and hi (d_hi).
// Sets: group g = the rows whose label is one of the `width` words of rows[g], the ascending distinct raw rows of the call (HOST
// memory, flattened); the walk reads every query's whole row of the DEVICE matrix d_sets, and d_group_of stays nullptr.
// Boxes: group g = the rows whose cells in the call's m named label columns lie within the m pairs of rows[g], the ascending distinct
// raw rows of 2m words (HOST memory, flattened; width = 2m); the walk reads every query's row of the DEVICE matrix d_sets likewise.
// n_bits is the shortest named column's cells.
// Boxes of 64-bit ends: the same with rows of 4m 32-bit words (label_box64_rows; width = 4m) over columns of either width.
// Set boxes: group g = the rows rows[g] admits, the ascending distinct travelling rows of 2 set_width + 4m words (label_set_box_rows;
// width = that, at most 76); `box` names the set column FIRST and the m range columns after it.
struct GroupedRows {
	const uint64_t *d_table = nullptr;  // bitmaps: n_groups bitmaps of n_bits bits
	uint64_t n_groups = 0, n_bits = 0;  // (labels: the distinct wanted values; the cells of the label column)
	const uint32_t *values = nullptr;   // labels: HOST
	const uint32_t *d_labels = nullptr; // labels: the label column
	const LabelRange *pairs = nullptr;  // ranges: HOST
	const uint32_t *group_of = nullptr, *d_group_of = nullptr;
	const uint32_t *d_hi = nullptr;     // ranges: every query's upper end (d_group_of holds the lower ends)
	const uint32_t *rows = nullptr;     // sets: HOST, n_groups x width
	const uint32_t *d_sets = nullptr;   // sets: the call's n_queries x width matrix
	uint32_t width = 0;                 // sets: words per row
	LabelBoxColumns box;                // boxes: the named columns
	uint32_t set_width = 0;             // set boxes: the words of a query's list

	static GroupedRows bitmaps(const uint64_t *d_table, uint64_t n_groups, uint64_t n_bits, HostWords group_of, DeviceWords d_group_of) {
		GroupedRows g;
		g.d_table = d_table, g.n_groups = n_groups, g.n_bits = n_bits, g.group_of = group_of.p, g.d_group_of = d_group_of.p;
		return g;
	}
	static GroupedRows labels(const std::vector<uint32_t> &values, const uint32_t *d_labels, uint64_t labelled_rows, HostWords group_of,
	                          DeviceWords d_want) {
		GroupedRows g;
		g.by_label = true, g.values = values.data(), g.d_labels = d_labels;
		g.n_groups = values.size(), g.n_bits = labelled_rows, g.group_of = group_of.p, g.d_group_of = d_want.p;
		return g;
	}
	static GroupedRows ranges(const std::vector<LabelRange> &pairs, const uint32_t *d_labels, uint64_t labelled_rows, HostWords group_of,
	                          DeviceWords d_lo, DeviceWords d_hi) {
		GroupedRows g;
		g.by_range = true, g.pairs = pairs.data(), g.d_labels = d_labels;
		g.n_groups = pairs.size(), g.n_bits = labelled_rows, g.group_of = group_of.p, g.d_group_of = d_lo.p, g.d_hi = d_hi.p;
		return g;
	}

	static GroupedRows sets(const std::vector<uint32_t> &rows, uint32_t width, const uint32_t *d_labels, uint64_t labelled_rows,
	                        HostWords group_of, DeviceWords d_sets) {
		GroupedRows g;
		g.by_set = true, g.rows = rows.data(), g.width = width, g.d_labels = d_labels;
		g.n_groups = rows.size() / width, g.n_bits = labelled_rows, g.group_of = group_of.p, g.d_sets = d_sets.p;
		return g;
	}

	static GroupedRows boxes(const std::vector<uint32_t> &rows, const LabelBoxColumns &box, HostWords group_of, DeviceWords d_boxes) {
		GroupedRows g;
		g.by_box = true, g.rows = rows.data(), g.width = 2 * box.m, g.box = box;
		g.n_groups = rows.size() / g.width, g.n_bits = box.shortest_rows(), g.group_of = group_of.p, g.d_sets = d_boxes.p;
		return g;
	}

	static GroupedRows boxes64(const std::vector<uint32_t> &rows, const LabelBoxColumns &box, HostWords group_of, DeviceWords d_boxes) {
		GroupedRows g;
		g.by_box64 = true, g.rows = rows.data(), g.width = 4 * box.m, g.box = box;
		g.n_groups = rows.size() / g.width, g.n_bits = box.shortest_rows(), g.group_of = group_of.p, g.d_sets = d_boxes.p;
		return g;
	}

	static GroupedRows set_boxes(const std::vector<uint32_t> &rows, uint32_t set_width, const LabelBoxColumns &box, HostWords group_of,
	                             DeviceWords d_rows) {
		GroupedRows g;
		g.by_set_box = true, g.rows = rows.data(), g.set_width = set_width, g.width = label_set_box_row_words(set_width, box.m - 1), g.box = box;
		g.n_groups = rows.size() / g.width, g.n_bits = box.shortest_rows(), g.group_of = group_of.p, g.d_sets = d_rows.p;
		return g;
	}

	// words that name one used group to the list kernels: its table group, its wanted value, the two ends of its range, the
	// words of its set, or the pairs of its box.  The walk of the graph-routed queries needs as many words per query gathered into
	// the compact batch.
	uint64_t group_cells() const {
		return by_set || by_box || by_box64 || by_set_box ? width : by_range ? 2 : 1;
	}
	// Those words beyond the one column k_route_gather takes along (d_group_of; under sets it takes none): `per` words a query,
	// row-major from `words`, to word `at` of the compact batch's ng * group_cells() words — or words == nullptr, nothing more.
	struct WalkWords {
		const uint32_t *words;
		uint32_t per;
		uint64_t at;
	};
	WalkWords more_walk_words(uint64_t ng) const {
		if (by_set || by_box || by_box64 || by_set_box)
			return {d_sets, width, 0};
		if (by_range)
			return {d_hi, 1, ng};
		return {nullptr, 0, 0};
	}

	// the list kernels' arguments in the label form: table group g is "the rows labelled values[g]", so the cells that name the
	// used groups hold their VALUES (ascending, as the groups are); the plan, its tables and the counts' layout are the same
	LabelListArgs label_list_args(const FilterListArgs &l) const {
		LabelListArgs a;
		a.keys = l.keys, a.rows = l.rows, a.n_blocks = l.n_blocks;
		a.labels = d_labels, a.labelled_rows = n_bits;
		a.values = l.groups, a.u_begin = l.u_begin, a.u_end = l.u_end;
		a.counts = l.counts, a.list_base = l.list_base, a.lists = l.lists;
		return a;
	}
	// ... and in the range form: the cells hold the groups' PAIRS, two words each
	RangeListArgs range_list_args(const FilterListArgs &l) const {
		RangeListArgs a;
		a.keys = l.keys, a.rows = l.rows, a.n_blocks = l.n_blocks;
		a.labels = d_labels, a.labelled_rows = n_bits;
		a.pairs = l.groups, a.u_begin = l.u_begin, a.u_end = l.u_end;
		a.counts = l.counts, a.list_base = l.list_base, a.lists = l.lists;
		return a;
	}
	// ... and in the set form: the cells hold the groups' ROWS, `width` words each
	SetListArgs set_list_args(const FilterListArgs &l) const {
		SetListArgs a;
		a.keys = l.keys, a.rows = l.rows, a.n_blocks = l.n_blocks;
		a.labels = d_labels, a.labelled_rows = n_bits;
		a.words = l.groups, a.width = width, a.u_begin = l.u_begin, a.u_end = l.u_end;
		a.counts = l.counts, a.list_base = l.list_base, a.lists = l.lists;
		return a;
	}
	// ... and in the box form: the cells hold the groups' ROWS, 2m words each
	BoxListArgs box_list_args(const FilterListArgs &l) const {
		BoxListArgs a = {};
		a.keys = l.keys, a.rows = l.rows, a.n_blocks = l.n_blocks;
		for (uint32_t j = 0; j != box.m; ++j)
			a.labels[j] = box.cells[j], a.labelled_rows[j] = box.rows[j];
		a.boxes = l.groups, a.u_begin = l.u_begin, a.u_end = l.u_end;
		a.counts = l.counts, a.list_base = l.list_base, a.lists = l.lists;
		return a;
	}
	// ... and in the 64-bit box form: 4m words each, and the columns' widths
	Box64ListArgs box64_list_args(const FilterListArgs &l) const {
		Box64ListArgs a = {};
		a.keys = l.keys, a.rows = l.rows, a.n_blocks = l.n_blocks;
		for (uint32_t j = 0; j != box.m; ++j)
			a.labels[j] = box.cells[j], a.labelled_rows[j] = box.rows[j];
		a.wide = box.wide_mask();
		a.boxes = l.groups, a.u_begin = l.u_begin, a.u_end = l.u_end;
		a.counts = l.counts, a.list_base = l.list_base, a.lists = l.lists;
		return a;
	}
	// ... and in the set-box form: travelling rows, the set column first among the columns
	SetBoxListArgs set_box_list_args(const FilterListArgs &l) const {
		SetBoxListArgs a = {};
		a.keys = l.keys, a.rows_n = l.rows, a.n_blocks = l.n_blocks;
		for (uint32_t j = 0; j != box.m; ++j)
			a.labels[j] = box.cells[j], a.labelled_rows[j] = box.rows[j];
		a.wide = box.wide_mask();
		a.rows = l.groups, a.width = set_width, a.u_begin = l.u_begin, a.u_end = l.u_end;
		a.counts = l.counts, a.list_base = l.list_base, a.lists = l.lists;
		return a;
	}
	// the cells of a plan's used groups, group_cells() words each: plan.groups, or their values / pairs / rows in `scratch` (which
	// outlives the upload like plan.groups)
	const uint32_t *used_group_cells(const ExactFilterPlan &plan, std::vector<uint32_t> &scratch) const {
		if (by_set || by_box || by_box64 || by_set_box) {
			scratch.resize((size_t)width * plan.groups.size());
			for (size_t u = 0; u != plan.groups.size(); ++u)
				std::copy(rows + (size_t)plan.groups[u] * width, rows + ((size_t)plan.groups[u] + 1) * width, scratch.begin() + u * width);
			return scratch.data();
		}
		if (by_range) {
			scratch.resize(2 * plan.groups.size());
			for (size_t u = 0; u != plan.groups.size(); ++u)
				scratch[2 * u] = pairs[plan.groups[u]].lo, scratch[2 * u + 1] = pairs[plan.groups[u]].hi;
			return scratch.data();
		}
		if (!by_label)
			return plan.groups.data();
		scratch.resize(plan.groups.size());
		for (size_t u = 0; u != scratch.size(); ++u)
			scratch[u] = values[plan.groups[u]];
		return scratch.data();
	}
	// step 1 of the listing: the block counts of used groups [l.u_begin, l.u_end)
	void launch_count(const FilterListArgs &l, hipStream_t stream) const {
		const dim3 grid((l.n_blocks + 3) / 4);
		if (by_label) { // (a wave writes the counts of the groups it meets only)
			HIP_TRY(hipMemsetAsync(l.counts, 0, (uint64_t)(l.u_end - l.u_begin) * l.n_blocks * 4, stream));
			hipLaunchKernelGGL(k_label_list_count, grid, dim3(256), 0, stream, label_list_args(l));
		} else if (by_range) // (every cell of the launch's groups is written)
			hipLaunchKernelGGL(k_range_list_count, grid, dim3(256), 0, stream, range_list_args(l));
		else if (by_set) // (the same)
			hipLaunchKernelGGL(k_set_list_count, grid, dim3(256), 0, stream, set_list_args(l));
		else if (by_box) // (the same; one kernel per number of named columns)
			switch (box.m) {
			case 1: hipLaunchKernelGGL(k_box_list_count<1>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			case 2: hipLaunchKernelGGL(k_box_list_count<2>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			case 3: hipLaunchKernelGGL(k_box_list_count<3>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			default: hipLaunchKernelGGL(k_box_list_count<4>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			}
		else if (by_box64)
			switch (box.m) {
			case 1: hipLaunchKernelGGL(k_box64_list_count<1>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			case 2: hipLaunchKernelGGL(k_box64_list_count<2>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			case 3: hipLaunchKernelGGL(k_box64_list_count<3>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			default: hipLaunchKernelGGL(k_box64_list_count<4>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			}
		else if (by_set_box) // (one kernel per number of range columns)
			switch (box.m - 1) {
			case 0: hipLaunchKernelGGL(k_set_box_list_count<0>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			case 1: hipLaunchKernelGGL(k_set_box_list_count<1>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			case 2: hipLaunchKernelGGL(k_set_box_list_count<2>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			default: hipLaunchKernelGGL(k_set_box_list_count<3>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			}
		else
			hipLaunchKernelGGL(k_filter_list_count, grid, dim3(256), 0, stream, l);
	}
	// step 3: the lists themselves, from the scanned counts
	void launch_scatter(const FilterListArgs &l, hipStream_t stream) const {
		const dim3 grid((l.n_blocks + 3) / 4);
		if (by_label)
			hipLaunchKernelGGL(k_label_list_scatter, grid, dim3(256), 0, stream, label_list_args(l));
		else if (by_range)
			hipLaunchKernelGGL(k_range_list_scatter, grid, dim3(256), 0, stream, range_list_args(l));
		else if (by_set)
			hipLaunchKernelGGL(k_set_list_scatter, grid, dim3(256), 0, stream, set_list_args(l));
		else if (by_box)
			switch (box.m) {
			case 1: hipLaunchKernelGGL(k_box_list_scatter<1>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			case 2: hipLaunchKernelGGL(k_box_list_scatter<2>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			case 3: hipLaunchKernelGGL(k_box_list_scatter<3>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			default: hipLaunchKernelGGL(k_box_list_scatter<4>, grid, dim3(256), 0, stream, box_list_args(l)); break;
			}
		else if (by_box64)
			switch (box.m) {
			case 1: hipLaunchKernelGGL(k_box64_list_scatter<1>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			case 2: hipLaunchKernelGGL(k_box64_list_scatter<2>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			case 3: hipLaunchKernelGGL(k_box64_list_scatter<3>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			default: hipLaunchKernelGGL(k_box64_list_scatter<4>, grid, dim3(256), 0, stream, box64_list_args(l)); break;
			}
		else if (by_set_box)
			switch (box.m - 1) {
			case 0: hipLaunchKernelGGL(k_set_box_list_scatter<0>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			case 1: hipLaunchKernelGGL(k_set_box_list_scatter<1>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			case 2: hipLaunchKernelGGL(k_set_box_list_scatter<2>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			default: hipLaunchKernelGGL(k_set_box_list_scatter<3>, grid, dim3(256), 0, stream, set_box_list_args(l)); break;
			}
		else
			hipLaunchKernelGGL(k_filter_list_scatter, grid, dim3(256), 0, stream, l);
	}
	// what the walk of a compact batch of ng graph-routed queries filters by; d_compact: their ng * group_cells() gathered words
	// (k_route_gather's column first, more_walk_words() where it says)
	SearchPredicate walk_predicate(const uint32_t *d_compact, uint64_t ng) const {
		const uint32_t *d_compact_groups = d_compact;
		if (by_set_box)
			return SearchPredicate::by_set_box(d_compact, set_width, box.columns, box.m, n_bits);
		if (by_box64)
			return SearchPredicate::by_box64(d_compact, box.columns, box.m, n_bits);
		if (by_box)
			return SearchPredicate::by_box(d_compact, box.columns, box.m, n_bits);
		if (by_set)
			return SearchPredicate::by_set(d_compact, width, n_bits);
		if (by_range)
			return SearchPredicate::by_range(d_compact_groups, d_compact + more_walk_words(ng).at, n_bits);
		if (by_label)
			return SearchPredicate::by_label(d_compact_groups, n_bits);
		return d_group_of ? SearchPredicate::one_table(d_table, d_compact_groups, n_groups, n_bits)
		                  : SearchPredicate::one_bitmap(d_table, n_bits);
	}

private:
	bool by_label = false, by_range = false, by_set = false, by_box = false, by_box64 = false, by_set_box = false;
	GroupedRows() = default;
};

// One batch in DEVICE memory: query q at d_queries + q * q_stride.  slot: the context that carries its walk, as SearchRequest's.
struct DeviceBatch {
	int slot;
	const float *d_queries;
	uint32_t q_stride;
	uint64_t nq, k, ef;
};
// ... and where its answers go, in DEVICE memory: k cells per query of keys / dist, one of count
struct DeviceAnswers {
	int64_t *keys;
	float *dist;
	uint32_t *count;
};
// One host-pointer call: what staged_call moves to and from a leased context (out_d, out_counts, out_route may be nullptr)
struct HostCall {
	const float *queries;
	uint64_t nq, k, ef;
	int64_t *out_keys;
	float *out_d;
	uint32_t *out_counts;
	uint8_t *out_route;
};

struct vss_index {
	// Reader/writer discipline of the reference (SURVEY §8b "Threading"): any number of concurrent searches (shared), every
	// call that changes the graph or its buffers exclusive.  Searches lease one of the pooled contexts below.
	std::shared_mutex rw;
	std::mutex stats_mu; // last_stats / last_query_stats / timing[0]
	int device = 0;
	hipStream_t stream = nullptr;
	bool own_stream = false;

	// configuration (reference hnsw_index.cpp:181-217)
	uint64_t dim = 0, M = 16, M0 = 32, efc = 128, efs = 64;
	int metric = 0;
	uint32_t V = 0, G = 1, logG = 0;
	uint64_t max_batch = 32768, growth_div = 32; // (round 3: cap 16384 -> 32768: fewer, larger phase-A launches, +5 % rows/s at 10M rows, recall unchanged)

	// host-side graph bookkeeping
	uint64_t limit_members = 0, limit_threads = 0;
	uint64_t capacity = 0;
	uint64_t count = 0;  // linked nodes (incl. tombstones)
	uint64_t staged = 0; // staged but not yet linked: slots [count, count + staged)
	int max_level = -1;
	uint32_t entry = 0;
	double inv_log_m = 0;
	LevelRng rng;
	std::vector<uint8_t> levels_h;
	std::vector<uint32_t> upper_off_h;
	std::vector<int64_t> keys_h;
	std::vector<uint32_t> list_owner_h;
	uint64_t n_upper = 0;
	uint64_t tombstones = 0;
	// some list may name a slot twice: a slot was re-used while stale links still pointed at it (or a loaded stream holds
	// such a list).  Decides how a chunk of a list goes through the visited set (mark_first_visit).
	bool lists_may_repeat = false;
	KeyMap keymap;
	FreeRing free_slots;
	std::atomic<uint64_t> progress_linked {0}, progress_total {0}; // vss_build_progress (read without the index lock)
	std::atomic<uint64_t> group_table_bytes {0}; // device bytes of the contexts' group tables (vss_memory_usage, read without a lock)

	// Staged rows that take over a tombstoned slot (the reference's update() path, index_dense.hpp:1766-1793): their
	// new vectors wait in d_pending until the node has been re-linked, because every distance to the slot taken during
	// that re-link still reads the OLD vector (index.hpp:2801-2859).  Once a reuse row is staged the row order of the
	// staged set is explicit: st_slot[i] = slot of staged row i, st_src[i] = its row in d_pending or EMPTY_SLOT.
	std::vector<uint32_t> st_slot, st_src;
	std::vector<int64_t> pending_keys;
	uint64_t n_pending = 0;
	DevBuf<float> d_pending;
	DevBuf<uint32_t> d_row_slot, d_row_src, d_parked;

	// device-side graph
	DevBuf<float> d_vectors;
	DevBuf<uint32_t> d_links0, d_links_up, d_upper_off, d_list_owner;
	DevBuf<uint8_t> d_levels;
	DevBuf<int64_t> d_keys;

	// The label column (label_filter.h): one 32-bit cell per ROW ID below `labelled_rows`, NO_LABEL where none was set.  By row
	// id like the callers' bitmaps, so slot reuse and vss_compact do not touch it; not serialized.  Written under the exclusive
	// lock only (vss_set_labels); d_labels.n may exceed labelled_rows (it grows by halves).
	DevBuf<uint32_t> d_labels;
	uint64_t labelled_rows = 0;
	// That is column 0 of LABEL_COLUMNS_MAX; columns 1 .. 3 are the same thing each (vss_set_label_column), read by the search by
	// label box only.  label_cells(c) / label_rows(c) name column c's pair.
	DevBuf<uint32_t> d_more_labels[LABEL_COLUMNS_MAX - 1];
	uint64_t more_labelled_rows[LABEL_COLUMNS_MAX - 1] = {};
	uint64_t label_column_bytes[LABEL_COLUMNS_MAX] = {};
	// A column's cells are 32 bits wide or 64 (vss_set_label_column64): 0 while it is empty, then the width of the setter that made
	// it, until it is cleared.  A 64-bit column keeps its cells in the same buffer, TWO words a cell (label_cells(c).n counts words),
	// and only the searches by label box64 and by label set box read it.
	uint32_t label_width[LABEL_COLUMNS_MAX] = {};
	std::atomic<uint64_t> label_bytes {0}; // every column's; vss_memory_usage (read without a lock)
	DevBuf<uint32_t> &label_cells(uint32_t column) {
		return column ? d_more_labels[column - 1] : d_labels;
	}
	uint64_t &label_rows(uint32_t column) {
		return column ? more_labelled_rows[column - 1] : labelled_rows;
	}

	// build scratch
	DevBuf<uint32_t> d_req_list, d_req_src, d_req_rank, d_sorted_src, d_touched, d_list_count, d_list_offset,
	    d_counters;
	DevBuf<float> d_req_d, d_sorted_d;
	uint32_t *h_counters = nullptr; // pinned
	DevBuf<uint32_t> d_node_status, d_work_build;
	DevBuf<float> d_build_list; // candidate lists in HBM (ef_construction > 512)
	uint32_t *h_debug = nullptr; // debug builds (-DVSS_PARANOID): 64 words of pinned host memory the kernels leave notes in
	DevBuf<unsigned long long> d_work_stats; // cumulative {phase A distances, phase A expansions, phase B distances}
	std::vector<uint32_t> h_node_status;

	// search contexts: independent in-flight batched probes over the same (read-only) graph — the analogue of usearch's
	// per-thread search contexts (index.hpp:2213-2240, leased in index_dense.hpp:1730-1745)
	struct SearchCtx {
		hipStream_t stream = nullptr;
		bool own_stream = false;
		DevBuf<uint32_t> d_stats, d_status, d_work, d_global_hash, d_retry_hash, d_queue;
		DevBuf<float> d_list_buf, d_cand_buf;
		uint32_t cand_cap = 0;
		// staging of the host-pointer entry points (one set per context, so that concurrent callers never share any)
		DevBuf<float> d_q, d_out_d;
		DevBuf<int64_t> d_out_keys;
		DevBuf<uint32_t> d_out_count;
		DevBuf<uint64_t> d_filter;
		DevBuf<uint64_t> d_group_filter; // vss_search_batch_filtered_groups: n_groups bitmaps end to end ...
		DevBuf<uint32_t> d_group_of;     // ... and the group of every query of the call
		DevBuf<const unsigned long long *> d_group_bitmap; // the address of every query's bitmap (either form of the call)
		uint64_t group_bytes = 0; // of these three, as counted in vss_index::group_table_bytes
		// vss_search_batch_filtered_groups_auto: the compact batch of the graph-routed queries and its answers
		DevBuf<float> d_route_q, d_route_d;
		DevBuf<int64_t> d_route_keys;
		DevBuf<uint32_t> d_route_group, d_route_count, d_route_map;
		unsigned char *pinned_io = nullptr;
		size_t pinned_cap = 0;
		bool leased = false;
		DevBuf<unsigned long long> d_phase;
		uint32_t *h_status = nullptr, *h_stats = nullptr; // pinned
		uint32_t *h_queue = nullptr; // pinned, written by the kernel: [1] engine error, [2] "last query handed out",
		                             // [3] queries answered (the flag wait of the one-query probe)
		bool flag_wait = false;      // this launch is waited for on h_queue[3], not on the stream; no events around it
		bool unsynced = false;       // a flag wait returned: the kernel's last instructions may still be in flight
		uint32_t flag_target = 0;    // h_queue[3] once this launch has answered all its queries (grows along a chain of launches)
		std::chrono::steady_clock::time_point flag_t0;
		uint32_t queue_sel = 0;      // which of the two query counters in d_queue the next launch takes
		size_t h_cap = 0;
		hipEvent_t ev0 = nullptr, ev1 = nullptr;
		bool pending = false;
		bool direct_io = false; // the kernel writes status / counters straight into the pinned host arrays
		SearchArgs args;
		uint64_t nq = 0, limit = 0, list_cap = 0;
		uint32_t bump = 0;
		uint32_t min_hash_log2 = 0; // after a visited-set overflow: the next pass's table is at least this large
		uint32_t shape[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // vss_last_search_shape: this call's first launch
		bool first_pass = true;
		double kernel_ms = 0;
		uint64_t stats[4] = {0, 0, 0, 0};
		// pre-scoring: the kernels add to d_prescore {rows pre-scored, rejected; the descent's rows handed over with a bound, those
		// that came back +inf} and never reset it; a call reports the difference
		DevBuf<unsigned long long> d_prescore;
		unsigned long long *h_prescore = nullptr; // pinned copy
		unsigned long long prescore_base[4] = {0, 0, 0, 0};
		bool prescore_first = false, prescore_used = false; // this call: its first launch filtered / any launch did
	};
	// contexts 0 .. EXPLICIT_CTX-1 belong to the caller (vss_search_batch_device_begin/_end; 0 is also the blocking
	// device-pointer calls' context and runs on the index stream); the rest are leased by the host-pointer entry points
	static constexpr int EXPLICIT_CTX = 4, MAX_CTX = 12;
	SearchCtx ctx[MAX_CTX];
	std::mutex lease_mu;
	std::condition_variable lease_cv;
	// after a context's group tables grew: keep the sum vss_memory_usage reports
	void count_group_tables(SearchCtx &c) {
		const uint64_t now = c.d_group_filter.n * 8 + c.d_group_of.n * 4 + c.d_group_bitmap.n * 8;
		group_table_bytes.fetch_add(now - c.group_bytes, std::memory_order_relaxed);
		c.group_bytes = now;
	}
	int lease_context() {
		std::unique_lock<std::mutex> lk(lease_mu);
		for (;;) {
			for (int i = EXPLICIT_CTX; i != MAX_CTX; ++i)
				if (!ctx[i].leased) {
					ctx[i].leased = true;
					return i;
				}
			lease_cv.wait(lk);
		}
	}
	void return_context(int i) {
		{
			std::lock_guard<std::mutex> lk(lease_mu);
			ctx[i].leased = false;
		}
		lease_cv.notify_one();
	}
	std::mutex ctx0_mu;  // blocking device-pointer searches share context 0
	std::mutex exact_mu; // the exact path's scratch (score tiles, norms) is shared: exact searches take turns
	std::mutex route_mu; // the routed device-pointer calls share context 0's compact batch

	// ---- row codes (row_codes.h): derived data of d_vectors for the scoring waves' pre-scoring (search.prescore, DESIGN.md §4.2, "Pre-scoring").
	// ONE mechanism keeps them valid: every path that writes rows marks its slots in `codes_stale` (or everything), and
	// ensure_codes() encodes what is marked — at the head of every search launch that would filter (nothing to do when clean)
	// and at the end of the calls that change rows, so that the first search does not pay.  Not serialized.
	// search.prescore, VSS_SEARCH_PRESCORE: 0 off (no codes held), 1 where it was measured to gain — limits of at most 256, the
	// 16-wave kernels —, 2 every pipelined launch (the 12-wave kernels of limits 257-512 too: measured SLOWER there)
	uint32_t search_prescore = 1;
	// search.prescore_descent, VSS_SEARCH_PRESCORE_DESCENT: the greedy descent's jobs carry closest_dist as their bound in the
	// launches that filter at all (1, the default); 0: they carry +inf, as every job of the descent did before
	bool search_prescore_descent = true;
	DevBuf<uint32_t> d_codes;        // capacity x V dwords
	DevBuf<RowCodeMeta> d_code_meta; // capacity
	StaleSlots codes_stale;
	std::mutex codes_mu;             // searches (shared index lock) encode stale slots one at a time
	uint64_t codes_refused_capacity = 0; // the capacity at which the device had no room for codes: not tried again until it changes
	uint64_t last_prescore[4] = {0, 0, 0, 0};
	uint64_t last_prescore_descent[2] = {0, 0}; // vss_last_search_prescore_descent
	// rows the instantiations with a pre-scoring path run at: full-wave rows of 2, 3, 4 or 6 chunks per lane
	bool codes_wanted() const {
		const uint32_t nch = (G == 64 && V % 64 == 0 && !force_looping) ? V / 64 : 0;
		return search_prescore && (nch == 2 || nch == 3 || nch == 4 || nch == 6);
	}
	void free_codes() {
		d_codes.free(), d_code_meta.free();
		codes_stale.clear();
		codes_refused_capacity = 0;
	}
	// true: the codes of every linked row (slots below `count`) are valid once `s` has run what this call put on it (it has:
	// the call waits).  may_allocate: only under the exclusive index lock — a search never replaces buffers another search
	// may be reading; it finds them too small (a reserve() since) and runs unfiltered.  No room on the device: no filter, no error.
	bool ensure_codes(hipStream_t s, bool may_allocate) {
		if (!codes_wanted() || !capacity)
			return false;
		std::lock_guard<std::mutex> lk(codes_mu);
		if (d_codes.n < capacity * V || d_code_meta.n < capacity) {
			if (!may_allocate || codes_refused_capacity == capacity)
				return false;
			HIP_TRY(hipStreamSynchronize(s));
			if (!d_codes.try_ensure(capacity * V) || !d_code_meta.try_ensure(capacity)) {
				d_codes.free(), d_code_meta.free();
				codes_refused_capacity = capacity;
				return false;
			}
			codes_stale.mark_all(); // (fresh buffers: undefined contents)
		}
		const StaleSlots before = codes_stale;
		uint64_t first = 0, end = 0;
		// rows that are staged but not linked stay marked: no search reads them, and their copies may still be in flight
		if (codes_stale.take(count, first, end)) {
			const uint32_t grid = (uint32_t)std::min<uint64_t>((end - first + 3) / 4, (uint64_t)n_cus * 16);
			hipLaunchKernelGGL(k_encode_rows, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4 *>(d_vectors.p), V, first, end,
			                   d_codes.p, d_code_meta.p);
			hipError_t status = hipGetLastError();
			if (status == hipSuccess)
				status = hipStreamSynchronize(s);
			if (status != hipSuccess) {
				codes_stale = before;
				throw HipError {status, "k_encode_rows"};
			}
		}
		return true;
	}

	// the same at the end of a call that changed rows (exclusive lock): codes are optional derived data, so a failure here
	// never fails the call that has already succeeded — the slots stay marked and searches run unfiltered until an encode succeeds
	void refresh_codes() noexcept {
		try {
			(void)ensure_codes(stream, true);
		} catch (...) {
			(void)hipGetLastError();
		}
	}

	// search scratch
	uint64_t last_stats[4] = {0, 0, 0, 0};
	uint32_t last_shape[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	std::vector<uint32_t> last_query_stats;
	// kernel timing (hipEvents on the index's stream): [0] last search kernel(s) ms, [1] build phase A ms,
	// [2] build phase B (count/alloc/scatter/link) ms, [3] build host wall ms, [4] build batches, [5] build retries
	double timing[6] = {0, 0, 0, 0, 0, 0};
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	void ensure_events() {
		for (auto &e : ev)
			if (!e)
				HIP_TRY(hipEventCreate(&e));
	}

	// exact-search scratch
	DevBuf<float> d_row_norm2, d_q_norm2, d_scores, d_best_s, d_qpad, d_cand_s;
	DevBuf<uint32_t> d_best_i, d_cand_cnt, d_cand_i, d_norm_ext, d_certified, d_redo_map;
	// 1 (default): a query whose selection by score is not certified (csrc/exact_certificate.h) is redone by brute force in the
	// metric; 2: every query is redone (tests)  (VSS_EXACT_CERTIFY).  exact_redo_qt: queries per workgroup of the redo kernel
	// (VSS_EXACT_REDO_QT; tests: the tiles it forms when fewer than MS_QT queries fit its LDS)
	uint32_t exact_certify = 1, exact_redo_qt = MS_QT;
	uint64_t last_exact_fallbacks = 0; // queries of the last exact call that were redone
	bool exact_filter = true; // the select folded into the score tile's epilogue from the second chunk on (VSS_EXACT_FILTER=0: A/B)
	uint64_t norms_valid_for = ~0ull; // value of `mutations` the norms were computed at
	// vss_search_exact_batch_filtered_groups (exact_filtered_kernels.h), under exact_mu like the rest: the lists of one pass, the
	// block counts of the groups in use, and the small tables of the plan.  exact_filter_budget = B, the entries the lists of
	// one pass may hold where that is more than the index has rows (VSS_EXACT_FILTER_LIST_ENTRIES).
	DevBuf<uint32_t> d_xf_lists, d_xf_counts, d_xf_tables;
	uint64_t exact_filter_budget = EXACT_FILTER_LIST_ENTRIES;
	uint64_t last_exact_filtered[4] = {0, 0, 0, 0}; // vss_last_exact_filtered
	uint64_t last_filter_route[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // vss_last_filter_route (under exact_mu too)
	std::atomic<uint64_t> exact_filter_bytes {0};   // of the three buffers (vss_memory_usage, read without a lock)
	uint64_t mutations = 0;

	int fail(const char *fmt, ...) {
		char buf[512];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(buf, sizeof buf, fmt, ap);
		va_end(ap);
		tls_error = buf;
		return VSS_ERROR;
	}

	uint32_t list_cap_max() const {
		return (uint32_t)((std::max(M, M0) + 63) / 64 * 64);
	}
	// limit of the insert search = config.expansion, as connect_node_across_levels_ passes it (usearch index.hpp:3648);
	// the max(max(M0, M) + 1, expansion) of index.hpp:2712-2713 is only the reservation of `top`
	uint32_t top_limit() const {
		return (uint32_t)std::max<uint64_t>(1, efc);
	}

	GraphView view() const {
		GraphView gv;
		gv.sp.vectors = reinterpret_cast<const float4 *>(d_vectors.p);
		gv.sp.V = V;
		gv.sp.G = G;
		gv.sp.logG = logG;
		gv.sp.metric = metric;
		gv.sp.debug_rows = (uint32_t)(count + staged);
		gv.sp.debug = h_debug;
		gv.dim = (uint32_t)dim;
		gv.M = (uint32_t)M;
		gv.M0 = (uint32_t)M0;
		gv.links0 = d_links0.p;
		gv.links_up = d_links_up.p;
		gv.upper_off = d_upper_off.p;
		gv.keys = d_keys.p;
		gv.list_id_base = (uint32_t)capacity;
		gv.filter = nullptr;
		gv.filter_bits = 0;
		gv.twins = lists_may_repeat ? 1u : 0u;
		return gv;
	}

	void release() {
		d_vectors.free(), d_links0.free(), d_links_up.free(), d_upper_off.free(), d_list_owner.free();
		d_levels.free(), d_keys.free();
		clear_labels();
		free_codes();
		d_req_list.free(), d_req_src.free(), d_req_rank.free(), d_sorted_src.free(), d_touched.free();
		d_list_count.free(), d_list_offset.free(), d_counters.free(), d_req_d.free(), d_sorted_d.free();
		d_node_status.free(), d_work_build.free(), d_work_stats.free(), d_build_list.free();
		if (h_debug)
			(void)hipHostFree(h_debug);
		h_debug = nullptr;
		d_pending.free(), d_row_slot.free(), d_row_src.free(), d_parked.free();
		d_global_hash.free(), d_row_norm2.free(), d_q_norm2.free(), d_scores.free(), d_best_s.free(), d_qpad.free();
		d_best_i.free(), d_cand_s.free(), d_cand_cnt.free(), d_cand_i.free();
		d_norm_ext.free(), d_certified.free(), d_redo_map.free();
		d_xf_lists.free(), d_xf_counts.free(), d_xf_tables.free();
		exact_filter_bytes.store(0, std::memory_order_relaxed);
		if (h_counters)
			(void)hipHostFree(h_counters);
		h_counters = nullptr;
		for (auto &e : ev) {
			if (e)
				(void)hipEventDestroy(e);
			e = nullptr;
		}
		for (auto &c : ctx) {
			if (c.unsynced && c.stream)
				(void)hipStreamSynchronize(c.stream);
			c.d_stats.free(), c.d_status.free(), c.d_work.free(), c.d_global_hash.free(), c.d_retry_hash.free(), c.d_phase.free();
			c.d_queue.free(), c.d_list_buf.free(), c.d_cand_buf.free();
			c.d_q.free(), c.d_out_d.free(), c.d_out_keys.free(), c.d_out_count.free(), c.d_filter.free();
			c.d_group_filter.free(), c.d_group_of.free(), c.d_group_bitmap.free();
			c.d_route_q.free(), c.d_route_d.free(), c.d_route_keys.free(), c.d_route_group.free(), c.d_route_count.free(), c.d_route_map.free();
			c.d_prescore.free();
			if (c.h_prescore)
				(void)hipHostFree(c.h_prescore);
			if (c.pinned_io)
				(void)hipHostFree(c.pinned_io);
			if (c.h_status)
				(void)hipHostFree(c.h_status), (void)hipHostFree(c.h_stats);
			if (c.h_queue)
				(void)hipHostFree(c.h_queue);
			if (c.ev0)
				(void)hipEventDestroy(c.ev0), (void)hipEventDestroy(c.ev1);
			if (c.own_stream && c.stream)
				(void)hipStreamDestroy(c.stream);
			c = SearchCtx();
		}
	}

	void reset_graph() {
		limit_members = limit_threads = capacity = count = staged = 0;
		max_level = -1;
		entry = 0;
		rng = LevelRng();
		levels_h.clear(), upper_off_h.clear(), keys_h.clear(), list_owner_h.clear();
		n_upper = tombstones = 0;
		lists_may_repeat = false;
		keymap = KeyMap();
		free_slots = FreeRing();
		st_slot.clear(), st_src.clear(), pending_keys.clear();
		n_pending = 0;
		mutations++;
	}

	// Mutating calls free or rewrite the arrays a search kernel of an unfinished begin/end probe may still be reading (its
	// stream is not the index stream): they are refused until every context has been completed with vss_search_batch_end.
	int refuse_while_probing(const char *what) {
		for (int i = 0; i != MAX_CTX; ++i)
			if (ctx[i].pending)
				return fail("%s while search context %d still has a batch in flight (call vss_search_batch_end first)", what, i);
		return VSS_OK;
	}

	// ------------------------------------------------------------------ the label column (label_filter.h)
	// the columns a call by label box names, as they are now: false where there are none or too many, one is out of range or named
	// twice, or one has never been set
	bool named_label_columns(const uint32_t *columns, uint64_t m, LabelBoxColumns &box) {
		if (m < 1 || m > LABEL_COLUMNS_MAX || !columns || label_box_bad_column(columns, (uint32_t)m) != m)
			return false;
		box.m = (uint32_t)m;
		for (uint32_t j = 0; j != box.m; ++j) {
			box.columns[j] = columns[j], box.cells[j] = label_cells(columns[j]).p, box.rows[j] = label_rows(columns[j]);
			box.width[j] = label_width[columns[j]];
			if (!box.cells[j])
				return false;
		}
		return true;
	}

	void clear_label_column(uint32_t column) {
		label_cells(column).free();
		label_rows(column) = 0;
		label_width[column] = 0;
		label_bytes.fetch_sub(label_column_bytes[column], std::memory_order_relaxed);
		label_column_bytes[column] = 0;
	}
	void clear_labels() { // every column
		for (uint32_t c = 0; c != LABEL_COLUMNS_MAX; ++c)
			clear_label_column(c);
	}

	// column `column`'s cells [first_rowid, first_rowid + n) = labels[0 .. n), from HOST or DEVICE memory; cells the write skips
	// over become NO_LABEL.  cell_words: 1 for 32-bit cells, 2 for 64-bit cells (`labels` then holds uint64_t, and the skipped
	// cells become NO_LABEL64); a column that has cells keeps their width.
	// Under the exclusive lock.  The column grows into a NEW buffer, and the old one goes only once the new one holds its cells: a
	// device without room fails this call and leaves the column as it was (nothing is visible before labelled_rows moves).
	int set_labels(const char *what, uint32_t column, uint64_t first_rowid, const void *labels, uint64_t n, bool on_device,
	               uint32_t cell_words = 1) {
		if (column >= LABEL_COLUMNS_MAX)
			return fail("%s: column %u is not below VSS_LABEL_COLUMNS_MAX (%u)", what, (unsigned)column, (unsigned)LABEL_COLUMNS_MAX);
		if (label_cells(column).p && label_width[column] != 32 * cell_words)
			return fail("%s: label column %u holds %u-bit cells and this call writes %u-bit cells (vss_clear_label_column it first)", what,
			            (unsigned)column, (unsigned)label_width[column], (unsigned)(32 * cell_words));
		const uint64_t cell_bytes = 4 * (uint64_t)cell_words;
		// (these two shadow column 0's members on purpose: what follows is the one column's code, for whichever column)
		DevBuf<uint32_t> &d_labels = label_cells(column);
		uint64_t &labelled_rows = label_rows(column);
		const LabelRangeFault fault = check_label_range(labels, first_rowid, n);
		if (fault == LabelRangeFault::NO_LABELS)
			return fail("%s: null label pointer", what);
		if (fault == LabelRangeFault::TOO_FAR)
			return fail("%s: %llu cells from row id %llu end beyond row id 2^32 - 1", what, (unsigned long long)n,
			            (unsigned long long)first_rowid);
		if (!n)
			return VSS_OK;
		if (refuse_while_probing(what) != VSS_OK)
			return VSS_ERROR;
		const LabelWrite w = label_write(labelled_rows, first_rowid, n);
		if (w.rows_after * cell_words > d_labels.n) {
			// by halves, so that a column written chunk by chunk next to the appends is not copied once per chunk
			const uint64_t roomy = std::min<uint64_t>(w.rows_after + w.rows_after / 2, LABEL_ROWS_MAX);
			uint32_t *np = nullptr;
			uint64_t got = roomy;
			if (hipMalloc(&np, roomy * cell_bytes) != hipSuccess) {
				(void)hipGetLastError();
				got = w.rows_after;
				if (hipMalloc(&np, got * cell_bytes) != hipSuccess) {
					(void)hipGetLastError();
					return fail("%s: no device memory for a label column of %llu rows (it keeps its %llu)", what,
					            (unsigned long long)w.rows_after, (unsigned long long)labelled_rows);
				}
			}
			hipError_t e = labelled_rows ? hipMemcpyAsync(np, d_labels.p, labelled_rows * cell_bytes, hipMemcpyDeviceToDevice, stream) : hipSuccess;
			if (e == hipSuccess)
				e = hipStreamSynchronize(stream);
			if (e != hipSuccess) {
				(void)hipFree(np);
				throw HipError {e, "label column growth"};
			}
			d_labels.free();
			d_labels.p = np, d_labels.n = got * cell_words;
			label_bytes.fetch_add(got * cell_bytes - label_column_bytes[column], std::memory_order_relaxed);
			label_column_bytes[column] = got * cell_bytes;
		}
		if (w.gap_end > w.gap_begin)
			HIP_TRY(hipMemsetAsync(d_labels.p + w.gap_begin * cell_words, 0xFF, (w.gap_end - w.gap_begin) * cell_bytes, stream)); // NO_LABEL(64)
		HIP_TRY(hipMemcpyAsync(d_labels.p + first_rowid * cell_words, labels, n * cell_bytes,
		                       on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		labelled_rows = w.rows_after;
		label_width[column] = 32 * cell_words;
		return VSS_OK;
	}

	// ------------------------------------------------------------------ reserve
	void ensure_upper(uint64_t lists) {
		if (lists <= d_links_up.n / std::max<uint64_t>(1, M))
			return;
		uint64_t want = std::max<uint64_t>(lists + lists / 2, 1024);
		d_links_up.ensure(want * M, n_upper * M, stream, 0xFF);
		d_list_owner.ensure(want, n_upper, stream);
	}

	int reserve(uint64_t members, uint64_t threads) {
		if (threads <= limit_threads && members <= limit_members)
			return VSS_OK;
		if (refuse_while_probing("vss_reserve") != VSS_OK)
			return VSS_ERROR;
		if (members >= 0x7FFFFFFFull)
			return fail("capacity above 2^31-1 slots is not supported");
		if (members < count + staged)
			return fail("cannot shrink below the number of stored vectors");
		limit_members = members;
		limit_threads = threads;
		const uint64_t live = count + staged;
		const uint64_t stride = (uint64_t)V * 4;
		d_vectors.ensure(members * stride, live * stride, stream, 0);
		d_links0.ensure(members * M0, live * M0, stream, 0xFF);
		d_upper_off.ensure(members, live, stream, 0);
		d_levels.ensure(members, live, stream, 0);
		d_keys.ensure(members, live, stream, 0);
		ensure_upper((uint64_t)(members / std::max<double>(1.0, (double)M - 1.0) * 1.25) + 1024);
		capacity = members;
		levels_h.resize(members, 0);
		upper_off_h.resize(members, 0);
		keys_h.resize(members, 0);
		rng = LevelRng(); // usearch replaces every thread context (and its generator) when it grows
		mutations++;
		return VSS_OK;
	}

	// ------------------------------------------------------------------ staging
	// Assign slots / levels for `n` valid rows whose keys are already in keys_h[first..], then upload metadata.
	int stage_metadata(uint64_t first, uint64_t n) {
		uint64_t upper_needed = n_upper;
		for (uint64_t i = 0; i != n; ++i) {
			const uint8_t lv = rng.stored_level(inv_log_m);
			levels_h[first + i] = lv;
			upper_off_h[first + i] = (uint32_t)upper_needed;
			upper_needed += lv;
		}
		ensure_upper(upper_needed);
		list_owner_h.resize(upper_needed);
		for (uint64_t i = 0; i != n; ++i)
			for (int l = 0; l < levels_h[first + i]; ++l)
				list_owner_h[upper_off_h[first + i] + l] = (uint32_t)(first + i);
		if (upper_needed > n_upper) {
			HIP_TRY(hipMemcpyAsync(d_list_owner.p + n_upper, list_owner_h.data() + n_upper,
			                       (upper_needed - n_upper) * 4, hipMemcpyHostToDevice, stream));
			HIP_TRY(hipMemsetAsync(d_links_up.p + n_upper * M, 0xFF, (upper_needed - n_upper) * M * 4, stream));
		}
		n_upper = upper_needed;
		HIP_TRY(hipMemcpyAsync(d_levels.p + first, levels_h.data() + first, n, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipMemcpyAsync(d_upper_off.p + first, upper_off_h.data() + first, n * 4, hipMemcpyHostToDevice,
		                       stream));
		HIP_TRY(hipMemcpyAsync(d_keys.p + first, keys_h.data() + first, n * 8, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipMemsetAsync(d_links0.p + first * M0, 0xFF, n * M0 * 4, stream));
		if (keymap.ready)
			for (uint64_t i = 0; i != n; ++i)
				keymap.put(keys_h[first + i], (uint32_t)(first + i));
		staged += n;
		mutations++;
		return VSS_OK;
	}

	int stage(const int64_t *rowids, const float *vecs, const uint64_t *validity, uint64_t n, bool device_ptrs) {
		if (!n)
			return VSS_OK;
		if (refuse_while_probing("vss_stage_batch") != VSS_OK)
			return VSS_ERROR;
		// which rows are valid (DuckDB validity mask: bit set = valid)
		const bool sparse = validity && !device_ptrs;
		std::vector<uint64_t> rows;
		if (sparse) {
			rows.reserve(n);
			for (uint64_t i = 0; i != n; ++i)
				if (validity[i >> 6] & (1ull << (i & 63)))
					rows.push_back(i);
		}
		const uint64_t nv = sparse ? rows.size() : n;
		if (!nv)
			return VSS_OK;
		// the keys of the valid rows, on the host
		std::vector<int64_t> kbuf(nv);
		if (device_ptrs) {
			HIP_TRY(hipMemcpyAsync(kbuf.data(), rowids, n * 8, hipMemcpyDeviceToHost, stream));
			HIP_TRY(hipStreamSynchronize(stream));
		} else if (!sparse) {
			std::memcpy(kbuf.data(), rowids, n * 8);
		} else {
			for (uint64_t i = 0; i != nv; ++i)
				kbuf[i] = rowids[rows[i]];
		}
		if (keymap.ready) { // duplicate check as usearch index_dense.hpp:1752-1753 (only when the map exists)
			uint32_t s;
			for (uint64_t i = 0; i != nv; ++i)
				if (keymap.find(kbuf[i], s))
					return fail("Duplicate keys not allowed in high-level wrappers");
		}
		// Slots: every add() first asks the free ring (index_dense.hpp:1767-1771), so the leading rows of the chunk take
		// over tombstoned slots in ring order until it runs dry; the rest are appended.
		std::vector<uint32_t> reused;
		{
			FreeRing before = free_slots;
			uint32_t s;
			while (reused.size() < nv && free_slots.try_pop(s))
				reused.push_back(s);
			if (count + staged + (nv - reused.size()) > capacity) { // usearch index.hpp:2728-2731
				free_slots = before;
				return fail("Reserve capacity ahead of insertions!");
			}
		}
		const uint64_t nr = reused.size(), first = count + staged;
		const size_t stride = (size_t)V * 4;
		const hipMemcpyKind kind = device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
		// copy the valid rows [a, b) of the chunk to consecutive padded rows at dst
		auto copy_rows = [&](uint64_t a, uint64_t b, float *dst) {
			if (a == b)
				return;
			if (!sparse) {
				HIP_TRY(hipMemcpy2DAsync(dst, stride * 4, vecs + a * dim, dim * 4, dim * 4, b - a, kind, stream));
				return;
			}
			for (uint64_t i = a; i < b;) { // runs of consecutive valid rows
				uint64_t j = i;
				while (j + 1 < b && rows[j + 1] == rows[j] + 1)
					j++;
				HIP_TRY(hipMemcpy2DAsync(dst + (i - a) * stride, stride * 4, vecs + rows[i] * dim, dim * 4, dim * 4,
				                         j - i + 1, kind, stream));
				i = j + 1;
			}
		};
		if (nr) {
			if (st_slot.empty()) // rows staged so far were all appended: make their order explicit
				for (uint64_t i = 0; i != staged; ++i)
					st_slot.push_back((uint32_t)(count + i)), st_src.push_back(EMPTY_SLOT);
			d_pending.ensure((n_pending + nr) * stride, n_pending * stride, stream, 0);
			copy_rows(0, nr, d_pending.p + n_pending * stride);
			for (uint64_t i = 0; i != nr; ++i) {
				st_slot.push_back(reused[i]), st_src.push_back((uint32_t)(n_pending + i));
				pending_keys.push_back(kbuf[i]);
				keys_h[reused[i]] = kbuf[i]; // the device copy stays FREE (invisible to searches) until the re-link
				if (keymap.ready)
					keymap.put(kbuf[i], reused[i]);
			}
			n_pending += nr;
			mutations++; // `tombstones` drops only when build_finalize has re-linked the slot and published its key on the device
		}
		int rc = VSS_OK;
		if (nv > nr) {
			copy_rows(nr, nv, d_vectors.p + first * stride);
			codes_stale.mark(first, first + (nv - nr));
			std::memcpy(keys_h.data() + first, kbuf.data() + nr, (nv - nr) * 8);
			if (!st_slot.empty())
				for (uint64_t i = 0; i != nv - nr; ++i)
					st_slot.push_back((uint32_t)(first + i)), st_src.push_back(EMPTY_SLOT);
			rc = stage_metadata(first, nv - nr);
		}
		if (!device_ptrs)
			HIP_TRY(hipStreamSynchronize(stream)); // the caller may recycle its chunk now
		return rc;
	}

	LaunchCfg launch_cfg(uint32_t grid, uint32_t lds, uint64_t list_limit) const {
		LaunchCfg c;
		c.nch = (V % G == 0 && !force_looping) ? V / G : 0; // chunks per lane when the row fills every lane evenly, else the looping kernels
		c.regs = (uint32_t)((list_limit + 63) / 64);
		c.grid = grid;
		c.lds = lds;
		c.threads = 64;
		c.stream = stream;
		return c;
	}
	template <typename A>
	void launch_by_metric(hipError_t (*f0)(const A &, const LaunchCfg &), hipError_t (*f1)(const A &, const LaunchCfg &),
	                      hipError_t (*f2)(const A &, const LaunchCfg &), const A &a, const LaunchCfg &c) const {
		HIP_TRY((metric == 0 ? f0 : metric == 1 ? f1 : f2)(a, c));
	}

	// Visited-set capacity: a level search touches roughly 16-35 x limit nodes (more with wide level-0 lists); the
	// table must stay below 7/8 full.  Tables above HASH_LDS_MAX_LOG2 live in HBM (see carve_lds).
	// Searches keep tables up to 32 KiB in LDS (measured faster at ef <= 128); the build keeps only <= 8 KiB there: with
	// the table in HBM/L2 phase A runs 8 instead of 3 waves per CU and is 1.6x faster (2M x 768, M=32).
	// The search engine (k_search): one persistent workgroup of `search_waves` waves per compute unit, the first
	// `search_walkers` of them walking one query each (0 = chosen per launch from the batch size), the rest scoring.
	// VSS_SEARCH_WAVES / VSS_SEARCH_WALKERS in the environment override them (A/B measurements).
	uint32_t search_waves = 16, search_walkers = 0;
	// walkers per workgroup the automatic choice may use (the kernel admits ENGINE_MAX_WALKERS = 8; VSS_SEARCH_WALKERS_CAP)
	uint32_t search_walkers_cap = 4;
	uint32_t search_wgs_per_cu = 1; // engine workgroups per compute unit (VSS_SEARCH_WGS_PER_CU; only with fewer than 16 waves each)
	// look-ahead while <= this many walkers of a workgroup still run (VSS_SEARCH_SPEC / vss_set_search_lookahead).  OFF by
	// default: bit-identical results, but measured slower — the probe sits on the walker's critical path
	uint32_t search_spec_active = 0;
	// The solo shape (k_search_solo: one wave per query scoring its own rows) answers launches of FEW queries over NARROW
	// rows — above all the single-query probe of HNSW_INDEX_SCAN: 0 = never, 1 = automatic (at most solo_max_queries
	// queries and a whole level-0 list of rows within solo_max_bytes: one wave pulls that about as fast as it could be
	// spread over scoring waves, without the exchange), 2 = always.  VSS_SEARCH_SOLO / VSS_SEARCH_SOLO_MAX override.
	uint32_t search_solo = 1, solo_max_queries = 32, solo_max_bytes = 32 * 1024;
	// The choice itself is pure host logic (host_logic.h: wants_solo / choose_search_shape, CPU-tested): narrow rows — one
	// wave pulls a whole level-0 list about as fast as it could be spread over scoring waves; as teams (helper waves behind
	// workgroup barriers) the shape wins while every query gets a compute unit of its own (1M x 128: 404 against 737 us for
	// 256 queries, profiles/r03t_engine_shapes_by_batch_1m128_touch_threshold.txt).
	// This is everything the index and its options contribute to a launch's plan (host_logic.h: plan_search_launch decides).
	host::SearchEngineConfig search_engine_config() const {
		host::SearchEngineConfig e;
		host::SearchShapePolicy &p = e.policy;
		p.solo_mode = search_solo, p.solo_max_queries = solo_max_queries, p.solo_max_bytes = solo_max_bytes;
		p.team = search_team, p.n_cus = n_cus;
		p.touch_rows = search_touch_rows, p.touch_lists = search_touch_lists, p.touch_max_queries = search_touch_max_queries;
		p.force_looping = force_looping;
		p.crew = search_crew, p.engine_walkers = search_walkers;
		e.M0 = M0, e.V = V, e.G = G, e.list_cap_max = list_cap_max(), e.nodes = count, e.hash_max_log2 = hash_max_log2();
		e.search_waves = search_waves, e.search_walkers_cap = search_walkers_cap, e.search_wgs_per_cu = search_wgs_per_cu;
		e.search_spec_active = search_spec_active, e.search_pipelined = search_pipelined, e.search_wide_lists = search_wide_lists;
		e.search_list_lds = search_list_lds, e.search_prescore = search_prescore, e.search_prescore_descent = search_prescore_descent;
		e.retry_in_place = retry_in_place, e.visited_per_limit = visited_per_limit;
		e.hash_lds_max_log2 = HASH_LDS_MAX_LOG2, e.hash_lds_max_override = hash_lds_max_override;
		e.visited_compact_on = visited_compact_on, e.search_crew_tune = search_crew_tune;
		return e;
	}
	// searches over tombstones / a predicate start with the register queue (VSS_SEARCH_REG_QUEUE=0: always the unbounded one)
	bool search_reg_queue = true;
	uint32_t reg_queue_max_limit = 64 * MAX_LIST_REGS; // (round 2: 256; VSS_SEARCH_REG_QUEUE_MAX for A/B)
	uint32_t n_cus = 256;
	bool force_looping = false; // VSS_FORCE_LOOPING=1: the looping (NCH = 0) kernels for every dimension (A/B of the unrolled ones)
	uint32_t exact_probe = 0; // VSS_EXACT_PROBE: timing diagnostics of the score tile (answers are wrong with it set)
	// score tile: 1 = round 2's (single LDS buffer), 2 / 3 = software-pipelined 128x128 / 128x256 (round 3), 4 = the 128x128 tile as
	// persistent workgroups staged through registers (round 5), 5 = the same with its operands brought in by LDS-DMA (the
	// default; dimensions that are no multiple of 32 run 4)  (VSS_EXACT_KERNEL)
	uint32_t exact_kernel = 5;
	uint32_t HASH_LDS_MAX_LOG2 = 13;
	uint32_t BUILD_HASH_LDS_MAX_LOG2 = 11;
	// a table of this size cannot overflow: every node fits below the 7/8 fill limit
	uint32_t hash_max_log2() const {
		return std::max<uint32_t>(10, log2u((count + staged + 2) * 8 / 7 + 64));
	}
	// sizing rule: host_logic.h (visited_set_log2, search_cells_per_limit; CPU-tested).  vss_set_search_visited_set (or
	// VSS_VISITED_PER_LIMIT / VSS_HASH_LDS_MAX_LOG2 / VSS_VISITED_COMPACT, read ONCE in vss_create) override the cells per
	// limit entry, the largest table LDS takes and the compact form for A/B measurements and tests.
	bool retry_in_place = true;          // overflowing LDS sets: the walker repeats the query over a table in HBM (SearchArgs::retry_hash)
	uint64_t visited_per_limit = 0;      // 0 = the rule's own
	uint32_t hash_lds_max_override = 0;  // 0 = HASH_LDS_MAX_LOG2
	bool visited_compact_on = true;
	uint32_t hash_log2_for(uint64_t limit, uint32_t bump, uint64_t per_limit = 64) const {
		if (visited_per_limit)
			per_limit = visited_per_limit;
		return host::visited_set_log2(limit, bump, M0, list_cap_max(), per_limit, hash_max_log2());
	}
	DevBuf<uint32_t> d_global_hash;
	uint32_t *global_hash_for(uint32_t hash_log2, uint64_t grid) {
		if (hash_log2 <= BUILD_HASH_LDS_MAX_LOG2)
			return nullptr;
		d_global_hash.ensure(grid << hash_log2, 0, stream);
		return d_global_hash.p;
	}

	void ensure_build_scratch(uint64_t batch, uint64_t max_lv) {
		// requests per node: <= M per level
		const uint64_t req_cap = batch * M * (max_lv + 1) + 64;
		d_req_list.ensure(req_cap, 0, stream), d_req_src.ensure(req_cap, 0, stream);
		d_req_rank.ensure(req_cap, 0, stream), d_req_d.ensure(req_cap, 0, stream);
		d_sorted_src.ensure(req_cap, 0, stream), d_sorted_d.ensure(req_cap, 0, stream);
		d_touched.ensure(req_cap, 0, stream);
		const uint64_t lists = capacity + d_list_owner.n;
		d_list_count.ensure(lists, 0, stream, 0);
		d_list_offset.ensure(lists, 0, stream, 0);
		d_counters.ensure(8, 0, stream, 0);
		d_work_stats.ensure(4, 0, stream, 0);
		if (!h_counters)
			HIP_TRY(hipHostMalloc((void **)&h_counters, 8 * sizeof(uint32_t), hipHostMallocDefault));
	}

	int build_finalize() {
		if (!staged && !n_pending)
			return VSS_OK;
		if (refuse_while_probing("vss_build_finalize") != VSS_OK)
			return VSS_ERROR;
		const bool reuse = !st_slot.empty(); // explicit row order: some rows take over tombstoned slots
		lists_may_repeat |= reuse;
		const uint64_t first = count, n = reuse ? st_slot.size() : staged;
		std::vector<uint8_t> lv_rows;
		if (reuse) {
			lv_rows.resize(n);
			for (uint64_t i = 0; i != n; ++i)
				lv_rows[i] = levels_h[st_slot[i]];
			d_row_slot.ensure(n, 0, stream), d_row_src.ensure(n, 0, stream);
			HIP_TRY(hipMemcpyAsync(d_row_slot.p, st_slot.data(), n * 4, hipMemcpyHostToDevice, stream));
			HIP_TRY(hipMemcpyAsync(d_row_src.p, st_src.data(), n * 4, hipMemcpyHostToDevice, stream));
		}
		const uint8_t *lv = reuse ? lv_rows.data() : levels_h.data() + first;
		auto slot_of = [&](uint64_t row) { return reuse ? (uint64_t)st_slot[row] : first + row; };
		uint64_t solo_row = ~0ull;
		for (uint64_t i = 0; reuse && i != n; ++i)
			if (st_src[i] != EMPTY_SLOT && st_slot[i] == entry)
				solo_row = i;
		std::vector<uint64_t> sizes = batch_schedule(first, max_level, lv, n, max_batch, growth_div, solo_row);
		uint64_t biggest = 0, top_lv = 0;
		for (uint64_t b : sizes)
			biggest = std::max(biggest, b);
		for (uint64_t i = 0; i != n; ++i)
			top_lv = std::max<uint64_t>(top_lv, lv[i]);
		ensure_build_scratch(biggest, top_lv);
		uint64_t appended = 0; // rows linked so far that extended the node count
		progress_linked.store(0, std::memory_order_relaxed);
		progress_total.store(n, std::memory_order_relaxed);
		// list ids of upper lists are offset by the capacity: the per-list scratch must cover them
		uint64_t done = 0;
		int rc = VSS_OK;
		ensure_events();
		bool pending_b = false;
		auto wall0 = std::chrono::steady_clock::now();
		for (uint64_t b : sizes) {
			const uint64_t slot0 = slot_of(done);
			if (slot0 == 0 && first == 0 && done == 0) { // the very first node just becomes the entry point (index.hpp:2749-2753)
				entry = 0;
				max_level = levels_h[0];
				done += b;
				count = first + (appended += b);
				progress_linked.store(done, std::memory_order_relaxed);
				continue;
			}
			uint32_t bump = 0;
			uint32_t level_hi = 0, batch_reused = 0;
			for (uint64_t j = 0; j != b; ++j) {
				level_hi = std::max<uint32_t>(level_hi, lv[done + j]);
				batch_reused += reuse && st_src[done + j] != EMPTY_SLOT;
			}
			BuildArgs reuse_args;
			if (batch_reused) { // update(): blank the tapes of the reused nodes before anybody searches (index.hpp:2837-2840)
				reuse_args.gv = view();
				reuse_args.levels = d_levels.p;
				reuse_args.max_level = max_level;
				reuse_args.list_cap_max = list_cap_max();
				reuse_args.row_slot = d_row_slot.p + done, reuse_args.row_src = d_row_src.p + done;
				reuse_args.parked_stride = (level_hi + 1) * list_cap_max();
				d_parked.ensure((uint64_t)b * reuse_args.parked_stride, 0, stream);
				reuse_args.parked = d_parked.p;
				hipLaunchKernelGGL(k_reuse_lists, dim3((uint32_t)b), dim3(64), 0, stream, reuse_args, 0);
			}
			HIP_TRY(hipMemsetAsync(d_counters.p, 0, 8 * sizeof(uint32_t), stream));
			d_node_status.ensure(b, 0, stream);
			if (h_node_status.size() < b)
				h_node_status.resize(b);
			std::vector<uint32_t> work;
			for (;;) {
				BuildArgs a;
				a.gv = view();
				a.first_slot = (uint32_t)slot0;
				a.n_nodes = (uint32_t)b;
				a.levels = d_levels.p;
				a.entry = entry;
				a.max_level = max_level;
				a.top_limit = top_limit();
				a.hash_log2 = hash_log2_for(top_limit(), bump);
				a.list_cap_max = list_cap_max();
				a.req_list = d_req_list.p, a.req_src = d_req_src.p, a.req_d = d_req_d.p;
				a.counters = d_counters.p;
				a.req_capacity = (uint32_t)d_req_list.n;
				const uint32_t grid = work.empty() ? (uint32_t)b : (uint32_t)work.size();
				a.global_hash = global_hash_for(a.hash_log2, grid);
				a.work = work.empty() ? nullptr : d_work_build.p;
				a.node_status = d_node_status.p;
				a.node_req_cap = (uint32_t)(M * (level_hi + 1));
				a.work_stats = d_work_stats.p;
				a.row_slot = reuse ? d_row_slot.p + done : nullptr;
				a.row_src = reuse ? d_row_src.p + done : nullptr;
				a.pending = reinterpret_cast<const float4 *>(d_pending.p);
				a.parked = batch_reused ? d_parked.p : nullptr;
				a.parked_stride = (level_hi + 1) * list_cap_max();
				const bool list_in_hbm = top_limit() > 64 * MAX_LIST_REGS; // ef_construction beyond the register lists
				a.cand_lds_cap = list_in_hbm ? 16 : a.top_limit;
				a.list_cap = list_in_hbm ? a.top_limit : 0;
				a.list_buf = nullptr;
				if (list_in_hbm) {
					d_build_list.ensure((uint64_t)grid * 2 * a.list_cap, 0, stream);
					a.list_buf = d_build_list.p;
				}
				const uint32_t lds = wave_lds_bytes(a.hash_log2, V, a.list_cap_max, a.cand_lds_cap, !a.global_hash) +
				                     align16(a.node_req_cap * 4) * 2;
				HIP_TRY(hipEventRecord(ev[0], stream));
				launch_by_metric<BuildArgs>(launch_phase_a<0>, launch_phase_a<1>, launch_phase_a<2>, a,
				                            launch_cfg(grid, lds, top_limit()));
				HIP_TRY(hipEventRecord(ev[1], stream));
				HIP_TRY(hipMemcpyAsync(h_counters, d_counters.p, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
				HIP_TRY(hipStreamSynchronize(stream));
				{
					float ms = 0;
					HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
					timing[1] += ms;
					if (pending_b) { // the previous batch's link kernels finished before this phase A started
						HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
						timing[2] += ms;
						pending_b = false;
					}
					timing[4] += 1;
				}
				if (!h_counters[3])
					break;
				// some nodes overflowed their visited set: re-run just those with a larger table
				if (a.hash_log2 >= hash_max_log2()) {
					rc = fail("visited-set overflow during build");
					break;
				}
				HIP_TRY(hipMemcpy(h_node_status.data(), d_node_status.p, b * 4, hipMemcpyDeviceToHost));
				std::vector<uint32_t> failed;
				if (work.empty()) {
					for (uint32_t j = 0; j != b; ++j)
						if (h_node_status[j])
							failed.push_back(j);
				} else {
					for (uint32_t j : work)
						if (h_node_status[j])
							failed.push_back(j);
				}
				work.swap(failed);
				timing[5] += work.size();
				d_work_build.ensure(b, 0, stream);
				HIP_TRY(hipMemcpyAsync(d_work_build.p, work.data(), work.size() * 4, hipMemcpyHostToDevice, stream));
				HIP_TRY(hipMemsetAsync(d_counters.p + 3, 0, sizeof(uint32_t), stream));
				bump += 2;
			}
			if (rc != VSS_OK)
				break;
			if (batch_reused)
				hipLaunchKernelGGL(k_reuse_lists, dim3((uint32_t)b), dim3(64), 0, stream, reuse_args, 1);
			const uint32_t n_req = h_counters[0];
			if (n_req) {
				LinkArgs l;
				l.gv = view();
				l.req_list = d_req_list.p, l.req_src = d_req_src.p, l.req_d = d_req_d.p, l.req_rank = d_req_rank.p;
				l.counters = d_counters.p;
				l.list_count = d_list_count.p, l.list_offset = d_list_offset.p, l.touched = d_touched.p;
				l.sorted_src = d_sorted_src.p, l.sorted_d = d_sorted_d.p;
				l.list_owner = d_list_owner.p, l.upper_off = d_upper_off.p;
				l.hash_log2 = 4; // phase B needs no visited set
				l.list_cap_max = list_cap_max();
				l.work_stats = d_work_stats.p;
				const uint32_t tb = 256, gb = std::min<uint32_t>((n_req + tb - 1) / tb, 2048);
				HIP_TRY(hipEventRecord(ev[2], stream));
				hipLaunchKernelGGL(k_link_count, dim3(gb), dim3(tb), 0, stream, l);
				hipLaunchKernelGGL(k_link_alloc, dim3(gb), dim3(tb), 0, stream, l);
				hipLaunchKernelGGL(k_link_scatter, dim3(gb), dim3(tb), 0, stream, l);
				const uint32_t lds = wave_lds_bytes(l.hash_log2, V, l.list_cap_max, l.list_cap_max + 1);
				launch_by_metric<LinkArgs>(launch_phase_b<0>, launch_phase_b<1>, launch_phase_b<2>, l,
				                           launch_cfg(std::min<uint32_t>(n_req, 65536), lds, 64));
				HIP_TRY(hipEventRecord(ev[3], stream));
				pending_b = true;
			}
			// update() epilogue: the new key, then the new vector (index.hpp:2850, index_dense.hpp:1777-1781) — stream
			// ordered after the link kernels, which still measured against the old vector
			for (uint64_t j = 0; batch_reused && j != b; ++j) {
				const uint32_t src = st_src[done + j], slot = st_slot[done + j];
				if (src == EMPTY_SLOT)
					continue;
				const uint64_t stride = (uint64_t)V * 4;
				HIP_TRY(hipMemcpyAsync(d_vectors.p + slot * stride, d_pending.p + src * stride, stride * 4,
				                       hipMemcpyDeviceToDevice, stream));
				codes_stale.mark(slot, (uint64_t)slot + 1);
				HIP_TRY(hipMemcpyAsync(d_keys.p + slot, &pending_keys[src], 8, hipMemcpyHostToDevice, stream));
			}
			// a node above the current top level is always a singleton batch: it becomes the entry (index.hpp:2769-2772)
			for (uint64_t j = 0; j != b; ++j) {
				if ((int)lv[done + j] > max_level) {
					max_level = lv[done + j];
					entry = (uint32_t)slot_of(done + j);
				}
			}
			for (uint64_t j = 0; j != b; ++j)
				appended += !reuse || st_src[done + j] == EMPTY_SLOT;
			tombstones -= batch_reused; // their keys are live on the device from here on (stream order)
			done += b;
			count = first + appended;
			progress_linked.store(done, std::memory_order_relaxed);
		}
		HIP_TRY(hipStreamSynchronize(stream));
		if (pending_b) {
			float ms = 0;
			HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
			timing[2] += ms;
		}
		timing[3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
		// rows of batches that did not run (error): plain appends stay staged; rows that were to take over a tombstoned slot
		// hand it back (the slot stays a tombstone: key, ring and rowid map as before the call)
		for (uint64_t i = done; reuse && i < n; ++i) {
			if (st_src[i] == EMPTY_SLOT)
				continue;
			const uint32_t slot = st_slot[i];
			if (keymap.ready)
				keymap.erase(keys_h[slot]);
			keys_h[slot] = VSS_FREE_KEY;
			if (free_slots.reserve(free_slots.size() + 1))
				free_slots.push(slot);
		}
		staged = first + staged - count;
		st_slot.clear(), st_src.clear(), pending_keys.clear();
		n_pending = 0;
		mutations++;
		// optional: finish a bulk build with the reference's compaction order (vss_set_build_reorder) — nodes of one cluster
		// contiguous in HBM; only when nothing is tombstoned (a build never prunes behind the caller's back)
		if (rc == VSS_OK && reorder_after_build && !tombstones && !staged && first == 0)
			rc = compact(true);
		return rc;
	}

	// ------------------------------------------------------------------ search
	SearchCtx &context(int slot) {
		SearchCtx &c = ctx[slot];
		if (!c.stream) {
			if (slot == 0) {
				c.stream = stream;
			} else {
				HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
				c.own_stream = true;
			}
			HIP_TRY(hipEventCreate(&c.ev0));
			HIP_TRY(hipEventCreate(&c.ev1));
			// (coherent whatever HIP_HOST_COHERENT says: the host spins on these words while the kernel that writes them still runs)
			HIP_TRY(hipHostMalloc((void **)&c.h_queue, 16, hipHostMallocCoherent));
		}
		if (slot == 0)
			c.stream = stream; // follows vss_set_stream
		return c;
	}

	// Launch the search engine over `n` queries (all of the batch, or the entries of args.work in a retry pass).
	void launch_search_kernel(SearchCtx &c, uint32_t n) {
		SearchArgs &a = c.args;
		a.n_queries = n;
		host::SearchLaunchInput in;
		in.n = n, in.limit = c.limit, in.bump = c.bump, in.min_hash_log2 = c.min_hash_log2;
		in.list_cap = c.list_cap, in.cand_cap = c.cand_cap, in.tomb = a.tomb, in.direct_io = c.direct_io;
		const host::SearchLaunchPlan plan = host::plan_search_launch(search_engine_config(), in);
		a.hash_log2 = plan.hash_log2, a.visited_compact = plan.visited_compact, a.stage_cap = plan.stage_cap;
		a.list_lds = plan.list_lds, a.walkers = plan.walkers;
		a.spec_active = plan.spec_active, a.touch_lines = plan.touch_lines, a.crew = plan.crew, a.pipelined = plan.pipelined;
		// pre-scoring on row codes (search.prescore), where the plan wants it and the codes can be had
		a.prescore = PrescoreView {nullptr, nullptr, nullptr};
		bool codes_ready = false;
		if (plan.wants_prescore) {
			try {
				codes_ready = ensure_codes(c.stream, false);
			} catch (const HipError &) { // (optional derived data: the search runs unfiltered, the slots stay marked)
				(void)hipGetLastError();
			}
		}
		if (codes_ready) {
			if (!c.d_prescore.p) {
				c.d_prescore.ensure(4, 0, c.stream, 0);
				HIP_TRY(hipHostMalloc((void **)&c.h_prescore, 4 * sizeof(unsigned long long), hipHostMallocDefault));
				for (int i = 0; i < 4; ++i)
					c.h_prescore[i] = 0, c.prescore_base[i] = 0;
			}
			a.prescore = PrescoreView {d_codes.p, d_code_meta.p, c.d_prescore.p};
			c.prescore_used = true;
		}
		// (the same launches, no others: without codes the kernel ignores it)
		a.prescore_descent = a.prescore.codes ? plan.prescore_descent : 0u;
		if (c.first_pass)
			c.prescore_first = a.prescore.codes != nullptr;
		// the scratch in HBM, to the plan's word counts
		a.global_hash = nullptr;
		if (plan.global_hash) {
			c.d_global_hash.ensure(plan.global_hash, 0, c.stream);
			a.global_hash = c.d_global_hash.p;
		}
		// the retry tables: no memory for them is no reason to fail a search that would have succeeded without — such queries
		// then go back to the host's re-run launch, as before round 5
		a.retry_hash = nullptr, a.retry_log2 = 0;
		if (plan.retry_hash && c.d_retry_hash.try_ensure(plan.retry_hash))
			a.retry_hash = c.d_retry_hash.p, a.retry_log2 = plan.retry_log2;
		a.list_cap = (uint32_t)c.list_cap;
		a.list_buf = nullptr;
		if (plan.list_buf) {
			c.d_list_buf.ensure(plan.list_buf, 0, c.stream);
			a.list_buf = c.d_list_buf.p;
		}
		a.cand_cap = c.cand_cap;
		a.cand_buf = nullptr;
		if (plan.cand_buf) {
			c.d_cand_buf.ensure(plan.cand_buf, 0, c.stream);
			a.cand_buf = c.d_cand_buf.p;
		}
		if (!c.d_queue.p) { // first launch on this context: both query counters start at zero
			c.d_queue.ensure(4 + 64, 0, c.stream);
			HIP_TRY(hipMemsetAsync(c.d_queue.p, 0, (4 + 64) * sizeof(uint32_t), c.stream));
			c.queue_sel = 0;
		}
		a.queue = c.d_queue.p;
		a.queue_sel = c.queue_sel;
		c.queue_sel ^= 2u;
		c.flag_wait = c.direct_io && probe_flag_wait;
		if (c.unsynced && !c.flag_wait) { // the previous launch was waited for by flag: let it retire before its words are reset
			HIP_TRY(hipStreamSynchronize(c.stream));
			c.unsynced = false;
		}
		a.engine_error = c.h_queue + 1;
		if (c.flag_wait) {
			// a chain of flag-waited launches never resets a pinned word (the previous kernel may still be retiring): the answer
			// count only grows, the error word is sticky, and nobody gates on such a launch
			if (!c.unsynced)
				c.h_queue[1] = 0, c.h_queue[3] = 0;
			a.drain_flag = nullptr;
			a.done_count = c.h_queue + 3;
		} else {
			c.h_queue[1] = 0, c.h_queue[2] = 0; // (this context has no launch in flight: nobody is writing them)
			a.drain_flag = c.h_queue + 2;
			a.done_count = nullptr;
		}
		LaunchCfg cfg;
		cfg.nch = plan.nch, cfg.regs = plan.regs, cfg.grid = plan.grid, cfg.lds = plan.lds_bytes, cfg.threads = plan.threads;
		cfg.stream = c.stream;
		if (c.first_pass) { // vss_last_search_shape
			std::memcpy(c.shape, plan.shape, sizeof c.shape);
			c.first_pass = false;
		}
		if (c.flag_wait)
			c.flag_t0 = std::chrono::steady_clock::now();
		else
			HIP_TRY(hipEventRecord(c.ev0, c.stream));
		if (plan.solo)
			launch_by_metric<SearchArgs>(launch_search_solo<0>, launch_search_solo<1>, launch_search_solo<2>, a, cfg);
		else
			launch_by_metric<SearchArgs>(launch_search<0>, launch_search<1>, launch_search<2>, a, cfg);
		if (c.flag_wait) // committed only now: a launch that failed above must not leave a target no kernel will ever reach
			c.flag_target = (c.unsynced ? c.flag_target : 0u) + n;
		else
			HIP_TRY(hipEventRecord(c.ev1, c.stream));
		if (!c.direct_io) {
			HIP_TRY(hipMemcpyAsync(c.h_status, c.d_status.p, c.nq * 4, hipMemcpyDeviceToHost, c.stream));
			HIP_TRY(hipMemcpyAsync(c.h_stats, c.d_stats.p, c.nq * 8, hipMemcpyDeviceToHost, c.stream));
		}
		if (a.prescore.codes)
			HIP_TRY(hipMemcpyAsync(c.h_prescore, c.d_prescore.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
	}

	// Pipelined launches (explicit contexts): a launch of the engine occupies every compute unit, so a second one issued
	// right away would only sit in its queue — and its clock (events, profilers) would run while it waits.  It is issued
	// when the previous one has handed out its last query, i.e. when compute units start to fall idle: the same overlap of
	// one launch's tail with the next one's body, and launch durations that mean execution.  Never waits longer than
	// the previous launch runs (its completion event ends the wait as well).
	bool search_gating = true;
	void wait_for_drain_of_previous_launch(int slot);
	// the pinned small-batch probe waits on a completion word in host memory (1) or on its stream, with events (0)
	bool probe_flag_wait = true;
	// solo shape: touch the rows of the cached neighbour lists one expansion ahead (launches of at most this many queries)
	bool search_touch_rows = true, search_touch_lists = true;
	uint32_t search_touch_max_queries = 256; // (measured up to one query per compute unit: 404 against 456 us for 256 queries)
	// solo shape with helper waves (teams), VSS_SEARCH_TEAM=0 for A/B
	bool search_team = true;
	// workgroup engine: crew mode for the last walker of a workgroup (vss_set_search_crew, VSS_SEARCH_CREW=0 for A/B)
	bool search_crew = true;
	// crew refinements (CREW_SPARE_SIMD | CREW_NO_REQUESTS bits; VSS_SEARCH_CREW_TUNE for A/B).  Both measured inside the
	// noise at 3M x 768 (profiles/r04d_*): off.
	uint32_t search_crew_tune = 0;
	// workgroup engine: software-pipelined level search (vss_set_search_pipelined, VSS_SEARCH_PIPELINED=0 for A/B)
	bool search_pipelined = true;
	// limits of 257-512 pipelined in 12-wave workgroups (vss_set_search_wide_lists, VSS_SEARCH_WIDE_LISTS=0 for A/B)
	bool search_wide_lists = true;
	// candidate lists of limits 513-4096 in LDS: 0 never, 1 automatic, 2 whenever a walker fits (search.list_lds, VSS_SEARCH_LIST_LDS)
	uint32_t search_list_lds = 1;

	// a request over rows of `dim` floats with no predicate and no option set: the callers name those field by field
	SearchRequest request(int slot, const float *const *d_queries, uint64_t n_batches, uint64_t per_batch, uint64_t k, uint64_t ef,
	                      int64_t *const *d_keys_out, float *const *d_dist_out, uint32_t *const *d_count_out) const {
		return {slot, n_batches, per_batch, d_queries, d_keys_out, d_dist_out, d_count_out, (uint32_t)dim, k, ef};
	}

	// The predicate of a launch by label whose batches each bring their own words (SearchPredicate::by_batches) becomes the walkers'
	// table HERE: one resolve kernel on the context's stream reads every batch's device matrices and writes the table of the kind
	// — the one the single-batch branches of search_begin write — for all n_batches * per_batch queries, into the context's
	// d_group_bitmap, sized for cap_q queries like the other per-query words.  Nothing is read back, copied or waited for.  The
	// re-run rounds of search_end read the table again by launch-wide query number, so a re-run query keeps its batch's predicate.
	// The six single-batch branches of search_begin keep their code for the blocking calls, so the choice of the flag bits and the
	// cut of the rows is written there AND here: a change to one must be made to the other until the blocking calls are re-pointed
	// at this path (the follow-up that also removes their host round trip).
	int resolve_label_batches(SearchCtx &c, const SearchPredicate &p, uint64_t n_batches, uint64_t per_batch, uint64_t cap_q, GraphView &gv) {
		LabelBatchShape s = {LabelKind::EQ, p.width, 0, (uint32_t)per_batch};
		uint64_t addresses[LABEL_COLUMNS_MAX] = {}, rows = labelled_rows, flags = 0;
		uint32_t wide_mask = 0;
		if (p.kind == SearchPredicate::BY_LABEL || p.kind == SearchPredicate::BY_RANGE || p.kind == SearchPredicate::BY_SET) {
			if (!d_labels.p || label_width[0] == 64 || (p.kind == SearchPredicate::BY_SET && (p.width < 1 || p.width > LABEL_SET_MAX)))
				return fail("search by label: over an index whose 32-bit labels have been set, set width 1 to %u", (unsigned)LABEL_SET_MAX);
			s.kind = p.kind == SearchPredicate::BY_LABEL ? LabelKind::EQ : p.kind == SearchPredicate::BY_RANGE ? LabelKind::RANGE : LabelKind::SET;
			flags = p.kind == SearchPredicate::BY_LABEL ? FILTER_BY_LABEL : p.kind == SearchPredicate::BY_RANGE ? FILTER_BY_RANGE : FILTER_BY_SET;
			addresses[0] = (uint64_t)reinterpret_cast<uintptr_t>(d_labels.p);
		} else {
			LabelBoxColumns box;
			const bool set_box = p.kind == SearchPredicate::BY_SET_BOX;
			if ((p.kind != SearchPredicate::BY_BOX && p.kind != SearchPredicate::BY_BOX64 && !set_box) ||
			    !named_label_columns(p.columns, p.n_columns, box) || (set_box && (p.width < 1 || p.width > LABEL_SET_MAX)))
				return fail("search by label box: over 1 to %u distinct label columns that have been set, set width 1 to %u",
				            (unsigned)LABEL_COLUMNS_MAX, (unsigned)LABEL_SET_MAX);
			wide_mask = box.wide_mask();
			if (p.kind == SearchPredicate::BY_BOX && wide_mask)
				return fail("search by label box: a named column holds 64-bit cells");
			s.kind = set_box ? LabelKind::SET_BOX : p.kind == SearchPredicate::BY_BOX ? LabelKind::BOX : LabelKind::BOX64;
			s.m = set_box ? box.m - 1 : box.m;
			flags = set_box ? FILTER_BY_SET_BOX : p.kind == SearchPredicate::BY_BOX ? FILTER_BY_BOX : FILTER_BY_BOX64;
			for (uint32_t j = 0; j != box.m; ++j)
				addresses[j] = (uint64_t)reinterpret_cast<uintptr_t>(box.cells[j]);
			rows = box.shortest_rows();
		}
		const uint64_t nq = n_batches * per_batch;
		if (!c.d_group_bitmap.try_grow(label_batches_table_cells(s, cap_q)))
			return fail("search by label: no device memory for the predicates of %llu queries", (unsigned long long)cap_q);
		count_group_tables(c);
		unsigned long long *table = reinterpret_cast<unsigned long long *>(c.d_group_bitmap.p);
		const LabelTableHead head = label_batches_table_head(s, addresses, wide_mask);
		const dim3 grid((uint32_t)(nq * label_batches_query_units(s) / 256 + 1));
		if (s.kind == LabelKind::BOX64 || s.kind == LabelKind::SET_BOX) {
			ResolveLabelBatchesArgs<uint64_t> res = {{}, s, head, (uint32_t)nq, table};
			for (uint64_t b = 0; b != n_batches; ++b)
				res.batch[b] = {static_cast<const uint64_t *>(p.label_words[b].words), static_cast<const uint64_t *>(p.label_words[b].lo),
				                static_cast<const uint64_t *>(p.label_words[b].hi)};
			hipLaunchKernelGGL(k_resolve_label_batches64, grid, dim3(256), 0, c.stream, res);
		} else {
			ResolveLabelBatchesArgs<uint32_t> res = {{}, s, head, (uint32_t)nq, table};
			for (uint64_t b = 0; b != n_batches; ++b)
				res.batch[b] = {static_cast<const uint32_t *>(p.label_words[b].words), static_cast<const uint32_t *>(p.label_words[b].lo),
				                static_cast<const uint32_t *>(p.label_words[b].hi)};
			hipLaunchKernelGGL(k_resolve_label_batches, grid, dim3(256), 0, c.stream, res);
		}
		HIP_TRY(hipGetLastError());
		gv.filter = table;
		// (the cut of the rows as the single-batch branches of search_begin make it: one bit lower per kind that took one)
		const uint64_t cut = p.kind == SearchPredicate::BY_LABEL ? FILTER_BY_LABEL : p.kind == SearchPredicate::BY_RANGE ? FILTER_BY_RANGE : FILTER_BY_SET;
		gv.filter_bits = std::min<uint64_t>(rows, cut - 1) | FILTER_PER_QUERY | flags;
		return VSS_OK;
	}

	// Enqueue the probe batches of a request on its context (asynchronous); search_end() completes them.  ONE launch of the
	// search engine answers all of them: its walkers take queries from every batch until none is left, so compute units that
	// drew short queries in one batch go on with the next instead of idling until the slowest query of the batch is done.
	int search_begin(const SearchRequest &r) {
		const int slot = r.slot;
		const uint64_t n_batches = r.n_batches, per_batch = r.per_batch, k = r.k;
		uint64_t ef = r.ef;
		if (slot < 0 || slot >= MAX_CTX)
			return fail("search context %d out of range (0..%d)", slot, MAX_CTX - 1);
		if (n_batches < 1 || n_batches > MAX_COALESCED)
			return fail("1 to %d batches per launch", MAX_COALESCED);
		SearchCtx &c = context(slot);
		if (c.pending)
			return fail("search context %d already has a batch in flight", slot);
		if (r.gate)
			wait_for_drain_of_previous_launch(slot);
		if (!ef)
			ef = efs ? efs : 64;
		const uint64_t limit = std::max(ef, k);
		if (k > 0x7FFFFFFFull || ef > 0x7FFFFFFFull)
			return fail("k / ef_search above 2^31-1");
		const uint64_t nq = n_batches * per_batch;
		if (nq > 0x7FFFFFFFull)
			return fail("more than 2^31-1 queries in one launch");
		c.stats[0] = c.stats[1] = c.stats[3] = 0;
		c.stats[2] = nq;
		c.kernel_ms = 0;
		c.nq = nq;
		c.prescore_first = c.prescore_used = false;
		if (!nq || !k)
			return VSS_OK;
		if (!count) { // empty index: no results (index.hpp:2895-2896)
			for (uint64_t b = 0; b != n_batches; ++b) {
				HIP_TRY(hipMemsetAsync(r.out_keys[b], 0xFF, per_batch * k * 8, c.stream));
				if (r.out_d[b])
					HIP_TRY(hipMemsetAsync(r.out_d[b], 0x7F, per_batch * k * 4, c.stream));
				HIP_TRY(hipMemsetAsync(r.out_count[b], 0, per_batch * 4, c.stream));
			}
			c.nq = 0;
			c.pending = true;
			return VSS_OK;
		}
		// the context's per-query words: sized ONCE for the largest launch the boundary admits at this batch size (a context that
		// has carried several batches will carry 32 — 12 bytes per query), not re-grown — device and pinned reallocations, each a
		// device-wide synchronisation — whenever a launch carries more batches than its predecessors (round 6: the driver's
		// 5 warm-up steps followed by 20 timed ones put exactly that inside the timed region: 2 % of it)
		const uint64_t cap_q = n_batches > 1 ? std::max<uint64_t>(nq, (uint64_t)MAX_COALESCED * per_batch) : nq;
		c.d_stats.ensure(cap_q * 2, 0, c.stream);
		c.d_status.ensure(cap_q, 0, c.stream);
		if (c.h_cap < nq) {
			if (c.h_status)
				(void)hipHostFree(c.h_status), (void)hipHostFree(c.h_stats);
			HIP_TRY(hipHostMalloc((void **)&c.h_status, cap_q * 4, hipHostMallocCoherent));
			HIP_TRY(hipHostMalloc((void **)&c.h_stats, cap_q * 8, hipHostMallocCoherent));
			c.h_cap = cap_q;
		}
		SearchArgs &a = c.args;
		a.gv = view();
		// The launch's predicate becomes the kernels' view of it HERE and nowhere else.  (Row ids are below 2^63 — 2^63 - 1 is the
		// free key — so a wider bitmap admits nothing more; the top bit is the kernels' FILTER_PER_QUERY.  The bit below it is
		// FILTER_BY_LABEL, which chooses the launch's kernels: a bitmap of 2^62 bits is 2^59 bytes, more than any address space
		// holds, so cutting a caller's n_bits there takes no row away that a bitmap in memory could admit.  FILTER_BY_RANGE took one
		// more bit, FILTER_BY_SET a fourth: the cut is at 2^60 - 1, a bitmap of 2^57 bytes — as much as a 57-bit address space holds
		// in all.)
		const SearchPredicate &p = r.predicate;
		a.gv.filter = p.kind == SearchPredicate::ONE_BITMAP ? reinterpret_cast<const unsigned long long *>(p.bitmap) : nullptr;
		a.gv.filter_bits = std::min<uint64_t>(p.n_bits, FILTER_BY_SET - 1);
		if (p.by_batches) {
			if (const int rc = resolve_label_batches(c, p, n_batches, per_batch, cap_q, a.gv))
				return rc;
		} else if (p.kind == SearchPredicate::PER_QUERY) {
			// Descriptor b = batch b's table.  A small kernel ahead of the launch resolves every query's bitmap address; the walkers
			// of the *_groups kernels read that (GraphView::admitted_for).  The descriptors go to it by value, so the launch path
			// allocates, copies and waits for nothing once the address table has its size — cap_q, like the other per-query words.
			if (!c.d_group_bitmap.try_grow(cap_q))
				return fail("filtered search: no device memory for the bitmap addresses of %llu queries", (unsigned long long)cap_q);
			count_group_tables(c);
			ResolveBatchesArgs res = {{}, filter_group_words(p.n_bits), (uint32_t)per_batch, (uint32_t)nq, c.d_group_bitmap.p};
			std::copy(p.batches, p.batches + n_batches, res.batch);
			hipLaunchKernelGGL(k_resolve_filter_group_batches, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, c.stream, res);
			HIP_TRY(hipGetLastError());
			a.gv.filter = reinterpret_cast<const unsigned long long *>(c.d_group_bitmap.p);
			a.gv.filter_bits |= FILTER_PER_QUERY;
		} else if (p.kind == SearchPredicate::BY_LABEL) {
			// The same table, read by the *_labels kernels (GraphView::admitted_label): cell 0 the column, then what every query's
			// rows must hold.  The re-run rounds of search_end read it again.
			if (n_batches != 1 || !d_labels.p)
				return fail("search by label: one batch per launch, over an index whose labels have been set");
			if (!c.d_group_bitmap.try_grow(cap_q + 1))
				return fail("search by label: no device memory for the wanted labels of %llu queries", (unsigned long long)cap_q);
			count_group_tables(c);
			ResolveLabelsArgs res = {d_labels.p, p.want, (uint32_t)nq, reinterpret_cast<unsigned long long *>(c.d_group_bitmap.p)};
			hipLaunchKernelGGL(k_resolve_label_wants, dim3((uint32_t)(nq / 256 + 1)), dim3(256), 0, c.stream, res);
			HIP_TRY(hipGetLastError());
			a.gv.filter = reinterpret_cast<const unsigned long long *>(c.d_group_bitmap.p);
			a.gv.filter_bits = std::min<uint64_t>(labelled_rows, FILTER_BY_LABEL - 1) | FILTER_PER_QUERY | FILTER_BY_LABEL;
		} else if (p.kind == SearchPredicate::BY_RANGE) {
			// ... and by the *_ranges kernels (GraphView::admitted_range): cell 0 the column, then two cells per query
			if (n_batches != 1 || !d_labels.p)
				return fail("search by label range: one batch per launch, over an index whose labels have been set");
			if (!c.d_group_bitmap.try_grow(2 * cap_q + 1))
				return fail("search by label range: no device memory for the ranges of %llu queries", (unsigned long long)cap_q);
			count_group_tables(c);
			ResolveRangesArgs res = {d_labels.p, p.lo, p.hi, (uint32_t)nq, reinterpret_cast<unsigned long long *>(c.d_group_bitmap.p)};
			hipLaunchKernelGGL(k_resolve_label_ranges, dim3((uint32_t)(nq / 256 + 1)), dim3(256), 0, c.stream, res);
			HIP_TRY(hipGetLastError());
			a.gv.filter = reinterpret_cast<const unsigned long long *>(c.d_group_bitmap.p);
			a.gv.filter_bits = std::min<uint64_t>(labelled_rows, FILTER_BY_RANGE - 1) | FILTER_PER_QUERY | FILTER_BY_RANGE;
		} else if (p.kind == SearchPredicate::BY_SET) {
			// ... and by the *_sets kernels (GraphView::admitted_set): cell 0 the column, cell 1 the width, then every query's
			// words in chunks of four, two cells a chunk
			if (n_batches != 1 || !d_labels.p || p.width < 1 || p.width > LABEL_SET_MAX)
				return fail("search by label set: one batch per launch, over an index whose labels have been set, width 1 to %u",
				            (unsigned)LABEL_SET_MAX);
			const uint64_t chunks = label_set_chunks(p.width);
			if (!c.d_group_bitmap.try_grow(2 * chunks * cap_q + 2))
				return fail("search by label set: no device memory for the sets of %llu queries", (unsigned long long)cap_q);
			count_group_tables(c);
			ResolveSetsArgs res = {d_labels.p, p.sets, (uint32_t)nq, p.width, reinterpret_cast<unsigned long long *>(c.d_group_bitmap.p)};
			hipLaunchKernelGGL(k_resolve_label_sets, dim3((uint32_t)(nq * 4 * chunks / 256 + 1)), dim3(256), 0, c.stream, res);
			HIP_TRY(hipGetLastError());
			a.gv.filter = reinterpret_cast<const unsigned long long *>(c.d_group_bitmap.p);
			a.gv.filter_bits = std::min<uint64_t>(labelled_rows, FILTER_BY_SET - 1) | FILTER_PER_QUERY | FILTER_BY_SET;
		} else if (p.kind == SearchPredicate::BY_BOX) {
			// ... and by the *_boxes kernels (GraphView::admitted_box): cell 0 the number of named columns, then their addresses,
			// then 2m cells per query.  No flag bit of its own: FILTER_BY_RANGE and FILTER_BY_SET together.
			LabelBoxColumns box;
			if (n_batches != 1 || !named_label_columns(p.columns, p.n_columns, box))
				return fail("search by label box: one batch per launch, over 1 to %u distinct label columns that have been set",
				            (unsigned)LABEL_COLUMNS_MAX);
			if (!c.d_group_bitmap.try_grow(label_box_table_cells(box.m, cap_q)))
				return fail("search by label box: no device memory for the boxes of %llu queries", (unsigned long long)cap_q);
			count_group_tables(c);
			ResolveBoxesArgs res = {};
			std::copy(box.cells, box.cells + box.m, res.columns);
			res.boxes = p.boxes, res.n_queries = (uint32_t)nq, res.m = box.m;
			res.table = reinterpret_cast<unsigned long long *>(c.d_group_bitmap.p);
			hipLaunchKernelGGL(k_resolve_label_boxes, dim3((uint32_t)(nq * box.m / 256 + 1)), dim3(256), 0, c.stream, res);
			HIP_TRY(hipGetLastError());
			a.gv.filter = reinterpret_cast<const unsigned long long *>(c.d_group_bitmap.p);
			a.gv.filter_bits = std::min<uint64_t>(box.shortest_rows(), FILTER_BY_SET - 1) | FILTER_PER_QUERY | FILTER_BY_BOX;
		} else if (p.kind == SearchPredicate::BY_BOX64) {
			// ... and by the *_boxes64 kernels (GraphView::admitted_box64): the head (the number of named columns and their
			// widths), their addresses, then 2m cells per query.  No flag bit of its own either: all three BY_ bits together.
			LabelBoxColumns box;
			if (n_batches != 1 || !named_label_columns(p.columns, p.n_columns, box))
				return fail("search by label box64: one batch per launch, over 1 to %u distinct label columns that have been set",
				            (unsigned)LABEL_COLUMNS_MAX);
			if (!c.d_group_bitmap.try_grow(label_box_table_cells(box.m, cap_q)))
				return fail("search by label box64: no device memory for the boxes of %llu queries", (unsigned long long)cap_q);
			count_group_tables(c);
			ResolveBoxes64Args res = {};
			std::copy(box.cells, box.cells + box.m, res.columns);
			res.boxes = p.boxes, res.n_queries = (uint32_t)nq, res.m = box.m, res.wide_mask = box.wide_mask();
			res.table = reinterpret_cast<unsigned long long *>(c.d_group_bitmap.p);
			hipLaunchKernelGGL(k_resolve_label_boxes64, dim3((uint32_t)(nq * box.m / 256 + 1)), dim3(256), 0, c.stream, res);
			HIP_TRY(hipGetLastError());
			a.gv.filter = reinterpret_cast<const unsigned long long *>(c.d_group_bitmap.p);
			a.gv.filter_bits = std::min<uint64_t>(box.shortest_rows(), FILTER_BY_SET - 1) | FILTER_PER_QUERY | FILTER_BY_BOX64;
		} else if (p.kind == SearchPredicate::BY_SET_BOX) {
			// ... and by the *_set_boxes kernels (GraphView::admitted_set_box): the head, the 1 + m addresses (set column first), then
			// every query's padded set words and 2m range cells.  No flag bit of its own: FILTER_BY_LABEL and FILTER_BY_SET without
			// FILTER_BY_RANGE.
			LabelBoxColumns box;
			if (n_batches != 1 || !named_label_columns(p.columns, p.n_columns, box) || p.width < 1 || p.width > LABEL_SET_MAX)
				return fail("search by label set box: one batch per launch, over 1 to %u distinct label columns that have been set, set "
				            "width 1 to %u", (unsigned)LABEL_COLUMNS_MAX, (unsigned)LABEL_SET_MAX);
			const uint32_t m = box.m - 1, padded = label_set_box_padded(p.width);
			if (!c.d_group_bitmap.try_grow(label_set_box_table_cells(m, padded, cap_q)))
				return fail("search by label set box: no device memory for the predicates of %llu queries", (unsigned long long)cap_q);
			count_group_tables(c);
			ResolveSetBoxesArgs res = {};
			std::copy(box.cells, box.cells + box.m, res.columns);
			res.rows = p.boxes, res.n_queries = (uint32_t)nq, res.width = p.width, res.m = m, res.wide_mask = box.wide_mask();
			res.table = reinterpret_cast<unsigned long long *>(c.d_group_bitmap.p);
			hipLaunchKernelGGL(k_resolve_label_set_boxes, dim3((uint32_t)(nq * label_set_box_query_cells(m, padded) / 256 + 1)), dim3(256), 0,
			                   c.stream, res);
			HIP_TRY(hipGetLastError());
			a.gv.filter = reinterpret_cast<const unsigned long long *>(c.d_group_bitmap.p);
			a.gv.filter_bits = std::min<uint64_t>(box.shortest_rows(), FILTER_BY_SET - 1) | FILTER_PER_QUERY | FILTER_BY_SET_BOX;
		}
		for (uint64_t b = 0; b != MAX_COALESCED; ++b) {
			const bool used = b < n_batches;
			a.queries[b] = used ? r.queries[b] : nullptr;
			a.out_keys[b] = used ? r.out_keys[b] : nullptr;
			a.out_d[b] = used ? r.out_d[b] : nullptr;
			a.out_count[b] = used ? r.out_count[b] : nullptr;
		}
		a.batch_size = (uint32_t)per_batch;
		a.q_stride = r.q_stride;
		a.n_queries = (uint32_t)nq;
		a.k = (uint32_t)k;
		a.ef = (uint32_t)ef;
		a.entry = entry;
		a.max_level = max_level;
		// rejected rows (tombstones, predicate) are traversed but not returned: the pending candidates wait in a register
		// queue while the limit allows (RegQueue), in the unbounded queue in HBM otherwise or once a query outgrew the former
		a.tomb = (tombstones || a.gv.filter) ? (limit <= reg_queue_max_limit && search_reg_queue ? 1u : 2u) : 0u;
		a.list_cap_max = list_cap_max();
		a.work = nullptr;
		c.direct_io = r.direct_io;
		a.out_stats = r.direct_io ? c.h_stats : c.d_stats.p;
		a.status = r.direct_io ? c.h_status : c.d_status.p;
		a.phase_ticks = nullptr;
#ifdef VSS_PHASE_TIMERS
		c.d_phase.ensure(nq * VSS_PHASE_STRIDE, 0, c.stream);
		a.phase_ticks = c.d_phase.p;
#endif
		c.limit = limit;
		c.bump = 0;
		c.min_hash_log2 = 0;
		c.first_pass = true;
		// beyond the register lists (ef_search or k above 512) the candidate list lives in HBM; no list outgrows the index
		c.list_cap = limit > 64 * MAX_LIST_REGS ? std::min<uint64_t>(limit, count) : 0;
		// accepted-but-unexpanded candidates of a search over tombstones / a predicate (the reference's unbounded `next` heap);
		// a query that outgrows the queue is re-run with a larger one
		c.cand_cap = (uint32_t)std::min<uint64_t>(count + 1, std::max<uint64_t>(1024, 4 * limit));
		if (r.direct_io)
			std::memset(c.h_status, 0xFF, nq * 4); // "not processed" until the engine says otherwise
		else
			HIP_TRY(hipMemsetAsync(c.d_status.p, 0xFF, nq * 4, c.stream));
		launch_search_kernel(c, (uint32_t)nq);
		c.pending = true;
		return VSS_OK;
	}

	int search_end(int slot, bool keep_query_stats) {
		if (slot < 0 || slot >= MAX_CTX)
			return fail("search context %d out of range", slot);
		SearchCtx &c = context(slot);
		if (!c.pending)
			return VSS_OK;
		c.pending = false;
		std::vector<uint32_t> work;
		int rounds = 0;
		for (;;) {
			if (c.flag_wait && c.nq) {
				// The one-query probe: ids, distances, counts and status are in pinned host memory, each query's published by a
				// system-scope release on h_queue[3].  Waiting on that word instead of on the stream saves the wake-up of
				// hipStreamSynchronize and the two event packets around the kernel; the stream is synchronised lazily, before
				// the context's next launch.  `search_kernel_ms` of such a call is the host clock from launch to flag.
				volatile uint32_t *done = c.h_queue + 3;
				bool seen = false;
				for (uint64_t spins = 0;; ++spins) {
					if ((int32_t)(*done - c.flag_target) >= 0) { // (wrap-safe: the count only grows)
						seen = true;
						break;
					}
					if ((spins & 1023) == 1023) {
						const auto waited = std::chrono::steady_clock::now() - c.flag_t0;
						if (waited > std::chrono::milliseconds(2)) { // far beyond any probe: let the stream decide
							if (hipStreamQuery(c.stream) != hipErrorNotReady)
								break; // finished without the flag (a failed launch), or done meanwhile: the stream decides
							std::this_thread::yield();
						}
					} else {
#if defined(__x86_64__) || defined(__i386__)
						__builtin_ia32_pause();
#else
						std::this_thread::yield();
#endif
					}
				}
				(void)hipGetLastError();
				std::atomic_thread_fence(std::memory_order_acquire);
				c.kernel_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c.flag_t0).count();
				if (seen) {
					c.unsynced = true;
				} else {
					HIP_TRY(hipStreamSynchronize(c.stream));
					c.unsynced = false; // (the next flag launch starts from zero again)
				}
			} else {
				HIP_TRY(hipStreamSynchronize(c.stream));
				c.unsynced = false;
			}
			if (!c.nq)
				break;
			if (!c.flag_wait) {
				float ms = 0;
				HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
				c.kernel_ms += ms;
			}
			if (c.h_queue[1])
				return fail("search engine: a walking wave gave up waiting for its scoring waves (internal error)");
#ifdef VSS_PARANOID
			{
				const uint32_t *note = h_debug;
				if (note[0])
					return fail("paranoid: %u bad chunks; first: c %u n %u id %u block %u wave %u ticket {n %u next %u} cnt %u last id %u",
					            note[0], note[1], note[2], note[3], note[4], note[5], note[6], note[7], note[8], note[9]);
			}
#endif
			work.clear();
			bool visited_full = false, queue_full = false;
			for (uint64_t i = 0; i != c.nq; ++i) {
				if (!c.h_status[i])
					continue;
				if (c.h_status[i] == LEVEL_OK_RETRIED) { // answered — by its walker's second attempt, over the table in HBM
					c.h_status[i] = LEVEL_OK;
					// counted once, among the re-run queries: in the first round only.  The device's status array is copied
					// back whole after every launch, so the word of a query that is NOT part of a later re-run round shows up
					// again there; a re-run query that its walker repeated once more is in `work` already.
					if (rounds == 0)
						c.stats[3] += 1;
					continue;
				}
				if (c.h_status[i] > LEVEL_QUEUE_OVERFLOW)
					return fail("search engine: query %llu was not processed (status %u; internal error)", (unsigned long long)i,
					            c.h_status[i]);
				work.push_back((uint32_t)i);
				visited_full |= c.h_status[i] == LEVEL_VISITED_OVERFLOW;
				queue_full |= c.h_status[i] == LEVEL_QUEUE_OVERFLOW;
			}
			if (work.empty())
				break;
			// some queries outgrew their scratch: re-run just those with more of it.  Both sizes are bounded by the number
			// of nodes (a visited set or a queue that holds every node cannot overflow), so this always terminates.
			if ((visited_full && c.args.hash_log2 >= hash_max_log2()) ||
			    (queue_full && c.args.tomb == 2 && c.cand_cap >= count + 1))
				return fail("search scratch overflow although sized for the whole index");
			if (++rounds > 64)
				return fail("search engine: scratch retries do not converge (internal error)");
			if (visited_full) {
				c.bump += 2;
				c.min_hash_log2 = std::max(c.args.hash_log2, c.args.retry_log2) + 1; // larger than anything these queries have had
			}
			if (queue_full) {
				if (c.args.tomb == 1)
					c.args.tomb = 2; // outgrew the register queue: the unbounded one
				else
					c.cand_cap = (uint32_t)std::min<uint64_t>(count + 1, (uint64_t)c.cand_cap * 8);
			}
			c.stats[3] += work.size();
			c.d_work.ensure(c.nq, 0, c.stream);
			HIP_TRY(hipMemcpyAsync(c.d_work.p, work.data(), work.size() * 4, hipMemcpyHostToDevice, c.stream));
			HIP_TRY(hipStreamSynchronize(c.stream)); // `work` is reused
			c.args.work = c.d_work.p;
			launch_search_kernel(c, (uint32_t)work.size());
		}
		for (uint64_t i = 0; i != c.nq; ++i) {
			c.stats[0] += c.h_stats[2 * i];
			c.stats[1] += c.h_stats[2 * i + 1];
		}
		{
			std::lock_guard<std::mutex> lk(stats_mu);
			std::memcpy(last_stats, c.stats, sizeof last_stats);
			std::memcpy(last_shape, c.shape, sizeof last_shape);
			last_prescore[0] = c.prescore_first ? 1 : 0;
			last_prescore[1] = last_prescore[2] = 0;
			if (c.prescore_used) {
				last_prescore[1] = c.h_prescore[0] - c.prescore_base[0];
				last_prescore[2] = c.h_prescore[1] - c.prescore_base[1];
				c.prescore_base[0] = c.h_prescore[0], c.prescore_base[1] = c.h_prescore[1];
			}
			last_prescore_descent[0] = last_prescore_descent[1] = 0;
			if (c.prescore_used) {
				last_prescore_descent[0] = c.h_prescore[2] - c.prescore_base[2];
				last_prescore_descent[1] = c.h_prescore[3] - c.prescore_base[3];
				c.prescore_base[2] = c.h_prescore[2], c.prescore_base[3] = c.h_prescore[3];
			}
			last_prescore[3] = d_codes.n * sizeof(uint32_t) + d_code_meta.n * sizeof(RowCodeMeta);
			timing[0] = c.kernel_ms;
			if (keep_query_stats)
				last_query_stats.assign(c.h_stats, c.h_stats + 2 * c.nq);
		}
		return VSS_OK;
	}

	// blocking search on the request's context (0 = the index stream, shared by the blocking device-pointer calls)
	int search_launch(const SearchRequest &r) {
		std::unique_lock<std::mutex> lk0(ctx0_mu, std::defer_lock);
		if (r.slot == 0)
			lk0.lock();
		int rc = search_begin(r);
		if (rc != VSS_OK)
			return rc;
		return search_end(r.slot, r.keep_query_stats);
	}

	struct Lease { // a pooled context for the duration of one host-pointer call
		vss_index *ix;
		int slot;
		explicit Lease(vss_index *i) : ix(i), slot(i->lease_context()) {
		}
		~Lease() {
			ix->ctx[slot].pending = false;
			ix->return_context(slot);
		}
	};

	// ---- staging of the host-pointer calls.  A table in HOST memory (group_of may be nullptr: none is staged) into buffers of the
	// leased context that grow and are reused.  No room on the device is an error of this call; the context keeps what it had.
	int stage_group_table(SearchCtx &c, const FilterGroupBatch &table, uint64_t n_bits, uint64_t nq) {
		const uint64_t words = table.n_groups * filter_group_words(n_bits);
		if (!c.d_group_filter.try_grow(std::max<uint64_t>(words, 1)) || (table.group_of && !c.d_group_of.try_grow(nq)))
			return fail("filtered search: no device memory for %llu bitmaps of %llu bits and the groups of %llu queries",
			            (unsigned long long)table.n_groups, (unsigned long long)n_bits, (unsigned long long)nq);
		count_group_tables(c);
		if (words)
			HIP_TRY(hipMemcpyAsync(c.d_group_filter.p, table.allowed, words * 8, hipMemcpyHostToDevice, c.stream));
		if (table.group_of)
			HIP_TRY(hipMemcpyAsync(c.d_group_of.p, table.group_of, nq * 4, hipMemcpyHostToDevice, c.stream));
		return VSS_OK;
	}
	// the wanted labels of a call by label (HOST memory): where a table's group numbers go, 4 bytes per query
	int stage_wanted_labels(SearchCtx &c, const uint32_t *want, uint64_t nq) {
		if (!c.d_group_of.try_grow(nq))
			return fail("search by label: no device memory for the wanted labels of %llu queries", (unsigned long long)nq);
		count_group_tables(c);
		HIP_TRY(hipMemcpyAsync(c.d_group_of.p, want, nq * 4, hipMemcpyHostToDevice, c.stream));
		return VSS_OK;
	}
	// the ends of a call by label range (HOST memory), in the same buffer: lo in words [0, nq), hi in [nq, 2 nq)
	int stage_label_ranges(SearchCtx &c, const uint32_t *lo, const uint32_t *hi, uint64_t nq) {
		if (!c.d_group_of.try_grow(2 * nq))
			return fail("search by label range: no device memory for the ranges of %llu queries", (unsigned long long)nq);
		count_group_tables(c);
		HIP_TRY(hipMemcpyAsync(c.d_group_of.p, lo, nq * 4, hipMemcpyHostToDevice, c.stream));
		HIP_TRY(hipMemcpyAsync(c.d_group_of.p + nq, hi, nq * 4, hipMemcpyHostToDevice, c.stream));
		return VSS_OK;
	}
	// the sets of a call by label set (HOST memory), in the same buffer: the nq x width matrix as it is
	int stage_label_sets(SearchCtx &c, const uint32_t *sets, uint32_t width, uint64_t nq) {
		if (!c.d_group_of.try_grow(nq * width))
			return fail("search by label set: no device memory for the sets of %llu queries", (unsigned long long)nq);
		count_group_tables(c);
		HIP_TRY(hipMemcpyAsync(c.d_group_of.p, sets, nq * width * 4, hipMemcpyHostToDevice, c.stream));
		return VSS_OK;
	}
	// the boxes of a call by label box (HOST memory), in the same buffer: the nq x 2m matrix as it is
	// (end_words: the 32-bit words of one end, 1, or 2 for the 64-bit ends of a call by label box64)
	int stage_label_boxes(SearchCtx &c, const uint32_t *boxes, uint32_t m, uint64_t nq, uint32_t end_words = 1) {
		if (!c.d_group_of.try_grow(nq * 2 * m * end_words))
			return fail("search by label box: no device memory for the boxes of %llu queries", (unsigned long long)nq);
		count_group_tables(c);
		HIP_TRY(hipMemcpyAsync(c.d_group_of.p, boxes, nq * 2 * m * end_words * 4, hipMemcpyHostToDevice, c.stream));
		return VSS_OK;
	}
	// the travelling rows of a call by label set box (HOST memory), in the same buffer: the nq x row_words matrix as it is
	int stage_label_set_boxes(SearchCtx &c, const uint32_t *rows, uint32_t row_words, uint64_t nq) {
		if (!c.d_group_of.try_grow(nq * row_words))
			return fail("search by label set box: no device memory for the predicates of %llu queries", (unsigned long long)nq);
		count_group_tables(c);
		HIP_TRY(hipMemcpyAsync(c.d_group_of.p, rows, nq * row_words * 4, hipMemcpyHostToDevice, c.stream));
		return VSS_OK;
	}
	// queries in, result buffers ensured ...
	void stage_queries(SearchCtx &c, const float *queries, uint64_t nq, uint64_t k) {
		c.d_q.ensure(nq * dim, 0, c.stream), c.d_out_count.ensure(nq, 0, c.stream);
		c.d_out_keys.ensure(nq * k, 0, c.stream), c.d_out_d.ensure(nq * k, 0, c.stream);
		HIP_TRY(hipMemcpyAsync(c.d_q.p, queries, nq * dim * 4, hipMemcpyHostToDevice, c.stream));
	}
	// ... results out, synchronised
	void fetch_results(SearchCtx &c, uint64_t nq, uint64_t k, int64_t *out_keys, float *out_d, uint32_t *out_counts) {
		HIP_TRY(hipMemcpyAsync(out_keys, c.d_out_keys.p, nq * k * 8, hipMemcpyDeviceToHost, c.stream));
		if (out_d)
			HIP_TRY(hipMemcpyAsync(out_d, c.d_out_d.p, nq * k * 4, hipMemcpyDeviceToHost, c.stream));
		if (out_counts)
			HIP_TRY(hipMemcpyAsync(out_counts, c.d_out_count.p, nq * 4, hipMemcpyDeviceToHost, c.stream));
		HIP_TRY(hipStreamSynchronize(c.stream));
	}
	// One host-pointer call answered through a leased context.  stage(c) puts the call's predicate into the context's buffers;
	// run(c, batch, answers, route) answers the staged batch into the context's result buffers and may fill `route`, a byte per
	// query, for hc.out_route.  on_index_stream: `run` launches on the index stream (the count and exact kernels do), so what was
	// staged on the context's stream has to have landed first.  A failure of either step returns before any answer is written.
	template <typename Stage, typename Run>
	int staged_call(const HostCall &hc, bool on_index_stream, Stage stage, Run run) {
		Lease lease(this);
		SearchCtx &c = context(lease.slot);
		if (const int rc = stage(c))
			return rc;
		stage_queries(c, hc.queries, hc.nq, hc.k);
		if (on_index_stream)
			HIP_TRY(hipStreamSynchronize(c.stream));
		std::vector<uint8_t> route;
		if (const int rc = run(c, DeviceBatch {lease.slot, c.d_q.p, (uint32_t)dim, hc.nq, hc.k, hc.ef},
		                       DeviceAnswers {c.d_out_keys.p, c.d_out_d.p, c.d_out_count.p}, route))
			return rc;
		fetch_results(c, hc.nq, hc.k, hc.out_keys, hc.out_d, hc.out_counts);
		if (hc.out_route)
			std::memcpy(hc.out_route, route.data(), hc.nq);
		return VSS_OK;
	}

	// `filter`: the predicate in HOST memory (of one batch: batches[0] where it has tables); exact search takes none
	static constexpr uint64_t DIRECT_IO_MAX_QUERIES = 256;
	int search_host(const float *queries, uint64_t nq, uint64_t k, uint64_t ef, int64_t *out_keys, float *out_d,
	                uint32_t *out_counts, bool exact, const SearchPredicate &filter) {
		if (!nq || !k)
			return VSS_OK;
		// Small batches — the one-query probe of HNSW_INDEX_SCAN (hnsw_index.cpp:315-356) and the chunks of HNSW_INDEX_JOIN
		// (hnsw_optimize_join.cpp:111-168; 204 queries at 768 dims): the kernel reads the queries from, and writes ids /
		// distances / counts / status straight into, one pinned host block.  No staging copies; the only host-device
		// interaction is the launch and one synchronisation.  (Up to DIRECT_IO_MAX_QUERIES — a query per compute unit: such a
		// launch is bound by its longest query, and a walker reads its 3 KiB over PCIe once per ~0.4 ms of work.)
		if (!exact && filter.kind == SearchPredicate::NONE && nq <= DIRECT_IO_MAX_QUERIES && count) {
			Lease lease(this);
			SearchCtx &c = context(lease.slot);
			const size_t q_bytes = (nq * dim * 4 + 15) & ~size_t(15), key_bytes = nq * k * 8;
			const size_t d_bytes = (nq * k * 4 + 15) & ~size_t(15), c_bytes = (nq * 4 + 15) & ~size_t(15);
			const size_t need = q_bytes + key_bytes + d_bytes + c_bytes;
			if (c.pinned_cap < need) {
				if (c.pinned_io)
					(void)hipHostFree(c.pinned_io);
				c.pinned_io = nullptr, c.pinned_cap = 0;
				HIP_TRY(hipHostMalloc((void **)&c.pinned_io, need, hipHostMallocCoherent));
				c.pinned_cap = need;
			}
			float *pq = reinterpret_cast<float *>(c.pinned_io);
			int64_t *pk = reinterpret_cast<int64_t *>(c.pinned_io + q_bytes);
			float *pd = reinterpret_cast<float *>(c.pinned_io + q_bytes + key_bytes);
			uint32_t *pc = reinterpret_cast<uint32_t *>(c.pinned_io + q_bytes + key_bytes + d_bytes);
			std::memcpy(pq, queries, nq * dim * 4);
			SearchRequest r = request(lease.slot, &pq, 1, nq, k, ef, &pk, &pd, &pc);
			r.direct_io = r.keep_query_stats = true;
			if (const int rc = search_launch(r))
				return rc;
			std::memcpy(out_keys, pk, nq * k * 8);
			if (out_d)
				std::memcpy(out_d, pd, nq * k * 4);
			if (out_counts)
				std::memcpy(out_counts, pc, nq * 4);
			return VSS_OK;
		}
		SearchPredicate staged; // the predicate of the launch: `filter`, in the context's buffers
		return staged_call(
		    {queries, nq, k, ef, out_keys, out_d, out_counts, nullptr}, exact,
		    [&](SearchCtx &c) -> int {
			    if (filter.kind == SearchPredicate::PER_QUERY) {
				    const FilterGroupBatch &table = filter.batches[0];
				    if (const int rc = stage_group_table(c, table, filter.n_bits, nq))
					    return rc;
				    staged = SearchPredicate::one_table(c.d_group_filter.p, c.d_group_of.p, table.n_groups, filter.n_bits);
			    } else if (filter.kind == SearchPredicate::ONE_BITMAP) {
				    const uint64_t words = filter_group_words(filter.n_bits);
				    c.d_filter.ensure(std::max<uint64_t>(words, 1), 0, c.stream);
				    HIP_TRY(hipMemcpyAsync(c.d_filter.p, filter.bitmap, words * 8, hipMemcpyHostToDevice, c.stream));
				    staged = SearchPredicate::one_bitmap(c.d_filter.p, filter.n_bits);
			    } else if (filter.kind == SearchPredicate::BY_LABEL) {
				    if (const int rc = stage_wanted_labels(c, filter.want, nq))
					    return rc;
				    staged = SearchPredicate::by_label(c.d_group_of.p, filter.n_bits);
			    } else if (filter.kind == SearchPredicate::BY_RANGE) {
				    if (const int rc = stage_label_ranges(c, filter.lo, filter.hi, nq))
					    return rc;
				    staged = SearchPredicate::by_range(c.d_group_of.p, c.d_group_of.p + nq, filter.n_bits);
			    } else if (filter.kind == SearchPredicate::BY_SET) {
				    if (const int rc = stage_label_sets(c, filter.sets, filter.width, nq))
					    return rc;
				    staged = SearchPredicate::by_set(c.d_group_of.p, filter.width, filter.n_bits);
			    } else if (filter.kind == SearchPredicate::BY_BOX) {
				    if (const int rc = stage_label_boxes(c, filter.boxes, filter.n_columns, nq))
					    return rc;
				    staged = SearchPredicate::by_box(c.d_group_of.p, filter.columns, filter.n_columns, filter.n_bits);
			    } else if (filter.kind == SearchPredicate::BY_BOX64) {
				    if (const int rc = stage_label_boxes(c, filter.boxes, filter.n_columns, nq, 2))
					    return rc;
				    staged = SearchPredicate::by_box64(c.d_group_of.p, filter.columns, filter.n_columns, filter.n_bits);
			    } else if (filter.kind == SearchPredicate::BY_SET_BOX) {
				    if (const int rc = stage_label_set_boxes(c, filter.boxes, label_set_box_row_words(filter.width, filter.n_columns - 1), nq))
					    return rc;
				    staged = SearchPredicate::by_set_box(c.d_group_of.p, filter.width, filter.columns, filter.n_columns, filter.n_bits);
			    }
			    return VSS_OK;
		    },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &) -> int {
			    if (exact)
				    return exact_launch(b.d_queries, b.q_stride, nq, k, out.keys, out.dist, out.count);
			    SearchRequest r = request(b.slot, &c.d_q.p, 1, nq, k, ef, &c.d_out_keys.p, &c.d_out_d.p, &c.d_out_count.p);
			    r.keep_query_stats = true;
			    r.predicate = staged;
			    return search_launch(r);
		    });
	}

	// ------------------------------------------------------------------ exact search
	int exact_launch(const float *d_queries, uint32_t q_stride, uint64_t nq, uint64_t k, int64_t *d_keys_out,
	                 float *d_dist_out, uint32_t *d_count_out) {
		const uint64_t rows = count;
		if (!nq || !k)
			return VSS_OK;
		std::lock_guard<std::mutex> exact_lock(exact_mu); // score tiles, norms and the index stream are shared
		last_exact_fallbacks = 0;
		// Contract: for finite inputs the answer is the brute force of the wave-order metric over the live rows,
		// ordered by (distance, slot).  Rows are SELECTED by an MFMA ranking score, the survivors re-scored with the metric; the
		// re-rank certifies per query that the selection cannot have lost a row (csrc/exact_certificate.h), and the queries it
		// cannot certify are redone with the metric itself as the score.
		// running top-(k + 8) per query; exact search is not reachable from the reference's SQL surface (HNSWIndex never passes
		// exact=true), its k is bounded by the select kernel's LDS
		if (k + 8 > SEL_KP_MAX)
			return fail("exact search supports k <= %d", SEL_KP_MAX - 8);
		const uint64_t KP = k + 8;
		if (!rows) {
			HIP_TRY(hipMemsetAsync(d_keys_out, 0xFF, nq * k * 8, stream));
			HIP_TRY(hipMemsetAsync(d_count_out, 0, nq * 4, stream));
			HIP_TRY(hipStreamSynchronize(stream));
			return VSS_OK;
		}
		const uint64_t CH = 32768;
		const uint64_t stride = (uint64_t)V * 4;
		d_row_norm2.ensure(capacity, 0, stream);
		d_qpad.ensure(nq * stride, 0, stream);
		d_q_norm2.ensure(nq, 0, stream);
		d_scores.ensure(nq * CH, 0, stream);
		d_best_s.ensure(nq * KP, 0, stream);
		d_best_i.ensure(nq * KP, 0, stream);
		d_norm_ext.ensure(2, 0, stream);
		d_certified.ensure(nq, 0, stream);
		if (norms_valid_for != mutations) {
			hipLaunchKernelGGL(k_row_norms, dim3(2048), dim3(256), 0, stream,
			                   reinterpret_cast<const float4 *>(d_vectors.p), V, G, logG, (uint32_t)rows, d_row_norm2.p);
			// the certificate's largest / smallest live |x|^2, cached with the norms
			HIP_TRY(hipMemsetAsync(d_norm_ext.p, 0, 4, stream));
			HIP_TRY(hipMemsetAsync(d_norm_ext.p + 1, 0xFF, 4, stream));
			hipLaunchKernelGGL(k_norm_extrema, dim3((uint32_t)std::min<uint64_t>((rows + 255) / 256, 1024)), dim3(256), 0, stream,
			                   d_row_norm2.p, d_keys.p, (uint32_t)rows, d_norm_ext.p);
			norms_valid_for = mutations;
		}
		HIP_TRY(hipMemsetAsync(d_qpad.p, 0, nq * stride * 4, stream));
		HIP_TRY(hipMemcpy2DAsync(d_qpad.p, stride * 4, d_queries, (size_t)q_stride * 4, dim * 4, nq,
		                         hipMemcpyDeviceToDevice, stream));
		hipLaunchKernelGGL(k_row_norms, dim3(256), dim3(256), 0, stream, reinterpret_cast<const float4 *>(d_qpad.p), V,
		                   G, logG, (uint32_t)nq, d_q_norm2.p);
		// Round 4: from the second chunk on the select is folded into the score tile's epilogue — only scores that beat a
		// query's K'-th best so far are kept (as survivors in a small per-query buffer), and the running top-K' is refreshed
		// from those buffers once per launch of eight chunks' worth of rows instead of from 128 KiB of scores per query after
		// every chunk.  Same answers:
		// a row is dropped only against a threshold that is never below the final one.  A query that collects more survivors
		// than its buffer holds (rows arriving in descending-distance order, say) raises a flag and the search is redone the
		// plain way.  VSS_EXACT_FILTER=0 keeps the plain way throughout (A/B).
		// How many rows a filtered launch may cover follows from the survivors it must expect: its threshold is the K'-th best
		// of the r0 rows seen so far, so a window of w rows in random order leaves about K' * w / r0 of them.  Windows are sized
		// to a quarter of the buffer (w <= r0 * CAND_CAP / (4 K'), at most eight chunks): k = 10 takes eight chunks from the
		// start, k = 200 grows its windows geometrically, and beyond K' = CAND_CAP / 8 (k > 248) — where even one chunk
		// behind one chunk would fill a quarter of the buffer — the plain way is taken from the start (the first
		// window of eight chunks used to overflow almost surely for k above ~248, and the whole pass was then repeated).
		const uint64_t CAND_CAP = SEL_CAP, SELECT_EVERY = 8;
		const bool want_filter = exact_filter && (exact_kernel == 2 || exact_kernel >= 4) && rows > CH && 8 * KP <= CAND_CAP;
		if (want_filter) {
			d_cand_cnt.ensure(nq + 1, 0, stream); // [nq] = the overflow flag
			d_cand_s.ensure(nq * CAND_CAP, 0, stream);
			d_cand_i.ensure(nq * CAND_CAP, 0, stream);
		}
		auto run = [&](bool filtered) {
			HIP_TRY(hipMemsetAsync(d_best_s.p, 0x7F, nq * KP * 4, stream)); // 0x7F7F7F7F = 3.39e38 (acts as +inf)
			HIP_TRY(hipMemsetAsync(d_best_i.p, 0xFF, nq * KP * 4, stream));
			if (filtered)
				HIP_TRY(hipMemsetAsync(d_cand_cnt.p, 0, (nq + 1) * 4, stream));
			// plain chunks are CH rows (the score matrix is nq x CH); a filtered launch stores no scores, so it covers
			// SELECT_EVERY chunks' worth of rows at once and is followed by one select over the survivors it left
			for (uint64_t r0 = 0; r0 < rows;) {
				const bool filter_this = filtered && r0 > 0;
				const uint64_t window = filter_this ? std::min(SELECT_EVERY * CH, std::max(CH, r0 * CAND_CAP / (4 * KP))) : CH;
				const uint64_t r1 = std::min(rows, r0 + window);
				ExactArgs e;
				e.queries = reinterpret_cast<const float4 *>(d_qpad.p);
				e.vectors = reinterpret_cast<const float4 *>(d_vectors.p);
				e.row_norm2 = d_row_norm2.p;
				e.query_norm2 = d_q_norm2.p;
				e.keys = d_keys.p;
				e.V = V;
				e.n_queries = (uint32_t)nq;
				e.row_begin = (uint32_t)r0;
				e.row_end = (uint32_t)r1;
				e.chunk_stride = (uint32_t)(filter_this ? r1 - r0 : CH);
				e.metric = metric;
				e.scores = d_scores.p;
				e.probe = exact_probe;
				e.best_s = d_best_s.p, e.best_i = d_best_i.p, e.KP = (uint32_t)KP, e.cand_cap = (uint32_t)CAND_CAP;
				e.cand_cnt = filter_this ? d_cand_cnt.p : nullptr;
				e.cand_s = d_cand_s.p, e.cand_i = d_cand_i.p;
				if (exact_kernel >= 4) { // round 5: the 128 x 128 tile as persistent workgroups, two per compute unit
					const uint64_t tiles = ((r1 - r0 + 127) / 128) * ((nq + 127) / 128);
					const uint32_t grid = (uint32_t)std::min<uint64_t>(2ull * n_cus, tiles);
					// operands by LDS-DMA (5, the default) where a row is a whole number of 128-byte steps and a tile's rows lie within
					// the 32-bit offsets of the DMA's address form; staged through registers (4) otherwise
					if (exact_kernel == 5 && V % 8 == 0 && 128ull * V * 16 < (1ull << 31)) {
						HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_exact_scores_v4), hipFuncAttributeMaxDynamicSharedMemorySize, (int)X4_LDS_BYTES));
						hipLaunchKernelGGL(k_exact_scores_v4, dim3(grid), dim3(256), X4_LDS_BYTES, stream, e);
					} else {
						const uint32_t lds = X2Shape<2>::LDS_BYTES;
						HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_exact_scores_v3), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
						hipLaunchKernelGGL(k_exact_scores_v3, dim3(grid), dim3(256), lds, stream, e);
					}
				} else if (exact_kernel >= 2) { // the software-pipelined tiles (round 3): 128 x 128 (2) or 128 x 256 (3)
					const bool wide = exact_kernel == 3;
					const uint32_t bn = wide ? X2Shape<4>::BN : X2Shape<2>::BN, lds = wide ? X2Shape<4>::LDS_BYTES : X2Shape<2>::LDS_BYTES;
					const void *fn = wide ? reinterpret_cast<const void *>(k_exact_scores_v2<4>) : reinterpret_cast<const void *>(k_exact_scores_v2<2>);
					HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
					dim3 grid((uint32_t)((r1 - r0 + bn - 1) / bn), (uint32_t)((nq + 127) / 128));
					if (wide)
						hipLaunchKernelGGL(k_exact_scores_v2<4>, grid, dim3(256), lds, stream, e);
					else
						hipLaunchKernelGGL(k_exact_scores_v2<2>, grid, dim3(256), lds, stream, e);
				} else {
					dim3 grid((uint32_t)((r1 - r0 + XT_BN - 1) / XT_BN), (uint32_t)((nq + XT_BM - 1) / XT_BM));
					hipLaunchKernelGGL(k_exact_scores, grid, dim3(XT_THREADS), 0, stream, e);
				}
				SelectArgs s;
				s.scores = filter_this ? nullptr : d_scores.p;
				s.chunk_stride = (uint32_t)CH;
				s.chunk_cols = (uint32_t)(r1 - r0);
				s.row_begin = (uint32_t)r0;
				s.KP = (uint32_t)KP;
				s.best_s = d_best_s.p;
				s.best_i = d_best_i.p;
				s.cand_cap = (uint32_t)CAND_CAP;
				s.cand_cnt = d_cand_cnt.p, s.cand_s = d_cand_s.p, s.cand_i = d_cand_i.p;
				s.overflow = d_cand_cnt.p ? d_cand_cnt.p + nq : nullptr;
				hipLaunchKernelGGL(k_exact_select, dim3((uint32_t)nq), dim3(SEL_THREADS), 0, stream, s);
				r0 = r1;
			}
		};
		run(want_filter);
		if (want_filter) {
			uint32_t overflowed = 0;
			HIP_TRY(hipMemcpyAsync(&overflowed, d_cand_cnt.p + nq, 4, hipMemcpyDeviceToHost, stream));
			HIP_TRY(hipStreamSynchronize(stream));
			if (overflowed)
				run(false);
		}
		RerankArgs r;
		r.gv = view();
		r.queries = d_queries;
		r.q_stride = q_stride;
		r.n_queries = (uint32_t)nq;
		r.k = (uint32_t)k;
		r.KP = (uint32_t)KP;
		r.best_i = d_best_i.p;
		r.out_keys = d_keys_out;
		r.out_d = d_dist_out;
		r.out_count = d_count_out;
		r.best_s = d_best_s.p;
		r.norm_ext = d_norm_ext.p;
		r.certified = d_certified.p;
		r.query_map = nullptr;
		const uint32_t lds = align16(V * 16) + 2 * align16((uint32_t)KP * 4);
		launch_by_metric<RerankArgs>(launch_rerank<0>, launch_rerank<1>, launch_rerank<2>, r,
		                             launch_cfg((uint32_t)nq, lds, 64));
		// the queries the re-rank could not certify: redone with the metric itself as the score
		std::vector<uint32_t> flags(nq), redo;
		HIP_TRY(hipMemcpyAsync(flags.data(), d_certified.p, nq * 4, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		for (uint64_t i = 0; i != nq; ++i)
			if (!flags[i] || exact_certify == 2)
				redo.push_back((uint32_t)i);
		last_exact_fallbacks = redo.size();
		if (redo.empty())
			return VSS_OK;
		const uint64_t nb = redo.size();
		d_redo_map.ensure(nb, 0, stream);
		HIP_TRY(hipMemcpyAsync(d_redo_map.p, redo.data(), nb * 4, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipMemsetAsync(d_best_s.p, 0x7F, nb * KP * 4, stream));
		HIP_TRY(hipMemsetAsync(d_best_i.p, 0xFF, nb * KP * 4, stream));
		MetricScoreArgs m;
		m.sp = r.gv.sp;
		m.keys = d_keys.p;
		m.queries = d_queries;
		m.q_stride = q_stride, m.dim = (uint32_t)dim;
		m.query_map = d_redo_map.p;
		m.n_map = (uint32_t)nb;
		m.qt = (uint32_t)std::min<uint64_t>(exact_redo_qt, (160 * 1024) / ((uint64_t)V * 16));
		if (!m.qt)
			return fail("exact search: a row of %llu dimensions does not fit the redo kernel's LDS", (unsigned long long)dim);
		m.chunk_stride = (uint32_t)CH;
		m.scores = d_scores.p;
		const uint32_t m_lds = m.qt * V * 16;
		const void *m_fn = metric == 0   ? reinterpret_cast<const void *>(k_exact_metric_scores<0>)
		                   : metric == 1 ? reinterpret_cast<const void *>(k_exact_metric_scores<1>)
		                                 : reinterpret_cast<const void *>(k_exact_metric_scores<2>);
		HIP_TRY(hipFuncSetAttribute(m_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<uint32_t>(m_lds, 64 * 1024)));
		for (uint64_t r0 = 0; r0 < rows; r0 += CH) {
			const uint64_t r1 = std::min(rows, r0 + CH);
			m.row_begin = (uint32_t)r0, m.row_end = (uint32_t)r1;
			const uint32_t rows_per_wave_pass = 64u >> logG;
			const uint64_t waves = (r1 - r0 + rows_per_wave_pass - 1) / rows_per_wave_pass;
			dim3 grid((uint32_t)std::min<uint64_t>((waves + 3) / 4, 8ull * n_cus), (uint32_t)((nb + m.qt - 1) / m.qt));
			if (metric == 0)
				hipLaunchKernelGGL(k_exact_metric_scores<0>, grid, dim3(256), m_lds, stream, m);
			else if (metric == 1)
				hipLaunchKernelGGL(k_exact_metric_scores<1>, grid, dim3(256), m_lds, stream, m);
			else
				hipLaunchKernelGGL(k_exact_metric_scores<2>, grid, dim3(256), m_lds, stream, m);
			SelectArgs s;
			s.scores = d_scores.p;
			s.chunk_stride = (uint32_t)CH;
			s.chunk_cols = (uint32_t)(r1 - r0);
			s.row_begin = (uint32_t)r0;
			s.KP = (uint32_t)KP;
			s.best_s = d_best_s.p;
			s.best_i = d_best_i.p;
			s.cand_cap = 0;
			s.cand_cnt = nullptr, s.cand_s = nullptr, s.cand_i = nullptr;
			s.overflow = nullptr;
			hipLaunchKernelGGL(k_exact_select, dim3((uint32_t)nb), dim3(SEL_THREADS), 0, stream, s);
		}
		r.certified = nullptr; // (the kept set is the metric's own top-K': nothing left to prove)
		r.query_map = d_redo_map.p;
		launch_by_metric<RerankArgs>(launch_rerank<0>, launch_rerank<1>, launch_rerank<2>, r,
		                             launch_cfg((uint32_t)nb, lds, 64));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(stream));
		return VSS_OK;
	}

	// ------------------------------------------------------------------ exact search under per-query predicates
	// Carries out the plan of exact_filtered_plan.h: list the live admitted slots of every group in use, score each query
	// against its group's list only, keep the K' smallest (distance, slot) pairs per query, re-rank.  Distances are the metric's
	// own from the start, so nothing is certified and nothing redone.  `g` names the groups, by bitmaps or by labels (GroupedRows).
	// In two steps, both under exact_mu, because the routed call (filtered_auto) decides between them which groups get lists.
	int exact_filtered_launch(const DeviceBatch &b, const GroupedRows &g, const DeviceAnswers &out) {
		std::lock_guard<std::mutex> exact_lock(exact_mu); // scores, running lists and the index stream are shared
		last_exact_fallbacks = 0;
		std::fill(last_exact_filtered, last_exact_filtered + 4, 0);
		if (b.k + 8 > SEL_KP_MAX)
			return fail("exact filtered search supports k <= %d", SEL_KP_MAX - 8);
		ExactFilterPlan plan;
		exact_filter_order(g.group_of, b.nq, g.n_groups, plan);
		std::vector<uint32_t> lengths;
		if (const int rc = exact_filtered_count(plan, b.nq, 1, g, lengths))
			return rc;
		return exact_filtered_score(plan, lengths, nullptr, b, g, out);
	}

	// d_xf_tables of a plan over nu used groups and nq queries: [groups nu x cells][totals nu] | [list_base nu][order nq][offset nq]
	// [length nq][tiles 5 x (<= nq)]; cells: the words that name a used group (GroupedRows::group_cells)
	struct ExactFilterTables {
		uint64_t at_totals, at_base, at_order, at_offset, at_length, at_tiles, words;
		ExactFilterTables(uint64_t nu, uint64_t nq, uint64_t cells)
		    : at_totals(cells * nu), at_base(at_totals + nu), at_order(at_base + nu), at_offset(at_order + nq), at_length(at_offset + nq),
		      at_tiles(at_length + nq), words(at_tiles + 5 * nq) {
		}
	};
	void count_exact_filter_scratch() {
		last_exact_filtered[3] = (d_xf_lists.n + d_xf_counts.n + d_xf_tables.n) * 4;
		exact_filter_bytes.store(last_exact_filtered[3], std::memory_order_relaxed);
	}
	FilterListArgs exact_filter_list_args(const GroupedRows &g, uint64_t nu, const ExactFilterTables &t) const {
		FilterListArgs l;
		l.keys = d_keys.p, l.rows = (uint32_t)count, l.n_blocks = (uint32_t)((count + FL_WAVE_SLOTS - 1) / FL_WAVE_SLOTS);
		l.table = g.d_table, l.words = filter_group_words(g.n_bits), l.n_bits = g.n_bits;
		l.groups = d_xf_tables.p, l.totals = d_xf_tables.p + t.at_totals, l.list_base = d_xf_tables.p + t.at_base;
		l.u_begin = 0, l.u_end = (uint32_t)nu;
		l.counts = d_xf_counts.p, l.lists = nullptr;
		return l;
	}
	// the cells of the used groups, to d_xf_tables (`scratch` outlives the copy like plan.groups)
	void upload_used_groups(const ExactFilterPlan &plan, const GroupedRows &g, std::vector<uint32_t> &scratch) {
		HIP_TRY(hipMemcpyAsync(d_xf_tables.p, g.used_group_cells(plan, scratch), plan.groups.size() * g.group_cells() * 4,
		                       hipMemcpyHostToDevice, stream));
	}

	// step 1: lengths[u] = live admitted rows of used group u of `plan` (a plan over nq queries); their block counts stay in
	// rows [0, nu) of d_xf_counts, which has room for count_copies times as many
	int exact_filtered_count(const ExactFilterPlan &plan, uint64_t nq, uint64_t count_copies, const GroupedRows &g,
	                         std::vector<uint32_t> &lengths) {
		const uint64_t nu = plan.groups.size(), rows = count;
		const ExactFilterTables t(nu, nq, g.group_cells());
		static_assert(sizeof(ExactFilterTile) == 20, "five words per tile");
		FilterListArgs l = exact_filter_list_args(g, nu, t);
		if (!d_xf_tables.try_grow(t.words) || !d_xf_counts.try_grow(std::max<uint64_t>(count_copies * nu * l.n_blocks, 1)))
			return fail("exact filtered search: no device memory for %llu queries over %llu groups in use", (unsigned long long)nq,
			            (unsigned long long)nu);
		l = exact_filter_list_args(g, nu, t); // (the buffers may have moved)
		count_exact_filter_scratch();
		ensure_events();
		HIP_TRY(hipEventRecord(ev[0], stream));
		lengths.assign(nu, 0);
		std::vector<uint32_t> values;
		if (nu && rows) { // (an empty index lists nothing: every length stays 0)
			upload_used_groups(plan, g, values);
			g.launch_count(l, stream);
			hipLaunchKernelGGL(k_filter_list_scan, dim3((uint32_t)nu), dim3(256), 0, stream, l);
			HIP_TRY(hipMemcpyAsync(lengths.data(), l.totals, nu * 4, hipMemcpyDeviceToHost, stream));
			HIP_TRY(hipStreamSynchronize(stream));
		}
		return VSS_OK;
	}

	// step 2: answers the queries plan.order names (rows of b.d_queries, cells of `out`) from lists of lengths[u] rows each.
	// taken_counts: nullptr where step 1 ran over this very plan (its groups and their scanned block counts are in place); else
	// row u = the scanned block counts of plan.groups[u], and the groups' cells are uploaded here.  No other query's cells are
	// written.
	int exact_filtered_score(ExactFilterPlan &plan, const std::vector<uint32_t> &lengths, uint32_t *taken_counts, const DeviceBatch &b,
	                         const GroupedRows &g, const DeviceAnswers &out) {
		const uint64_t k = b.k;
		if (k + 8 > SEL_KP_MAX)
			return fail("exact filtered search supports k <= %d", SEL_KP_MAX - 8);
		const uint32_t qt = (uint32_t)std::min<uint64_t>(MS_QT, (160 * 1024) / ((uint64_t)V * 16));
		if (!qt)
			return fail("exact filtered search: a row of %llu dimensions does not fit the scoring kernel's LDS", (unsigned long long)dim);
		const uint64_t KP = k + 8, CH = 32768, rows = count, nq = plan.order.size(), nu = plan.groups.size();
		if (!nq)
			return VSS_OK;
		const ExactFilterTables t(nu, nq, g.group_cells());
		const uint64_t at_base = t.at_base, at_order = t.at_order, at_offset = t.at_offset, at_length = t.at_length, at_tiles = t.at_tiles;
		if (!d_xf_tables.try_grow(t.words) || !d_scores.try_grow(nq * CH) || !d_best_s.try_grow(nq * KP) || !d_best_i.try_grow(nq * KP))
			return fail("exact filtered search: no device memory for %llu queries over %llu groups in use", (unsigned long long)nq,
			            (unsigned long long)nu);
		HIP_TRY(hipMemsetAsync(d_best_s.p, 0x7F, nq * KP * 4, stream)); // 0x7F7F7F7F = 3.39e38 (acts as +inf)
		HIP_TRY(hipMemsetAsync(d_best_i.p, 0xFF, nq * KP * 4, stream));
		FilterListArgs l = exact_filter_list_args(g, nu, t);
		std::vector<uint32_t> values;
		if (taken_counts) {
			l.counts = taken_counts;
			if (nu) // (plan.groups and `values` outlive the copy: this step ends synchronised)
				upload_used_groups(plan, g, values);
		}
		exact_filter_pack(lengths.data(), std::max<uint64_t>(exact_filter_budget, rows), qt, plan);
		uint64_t entries_max = 0;
		for (const ExactFilterPass &pass : plan.passes)
			entries_max = std::max(entries_max, pass.entries);
		if (!d_xf_lists.try_grow(std::max<uint64_t>(entries_max, 1)))
			return fail("exact filtered search: no device memory for lists of %llu rows", (unsigned long long)entries_max);
		count_exact_filter_scratch();
		last_exact_filtered[0] = plan.listed, last_exact_filtered[1] = plan.distances, last_exact_filtered[2] = plan.passes.size();
		{
			std::vector<uint32_t> up(at_tiles - at_base + 5 * plan.tiles.size());
			std::copy(plan.list_base.begin(), plan.list_base.begin() + nu, up.begin());
			std::copy(plan.order.begin(), plan.order.end(), up.begin() + (at_order - at_base));
			std::copy(plan.query_offset.begin(), plan.query_offset.end(), up.begin() + (at_offset - at_base));
			std::copy(plan.query_length.begin(), plan.query_length.end(), up.begin() + (at_length - at_base));
			if (!plan.tiles.empty())
				std::memcpy(up.data() + (at_tiles - at_base), plan.tiles.data(), plan.tiles.size() * sizeof(ExactFilterTile));
			HIP_TRY(hipMemcpyAsync(d_xf_tables.p + at_base, up.data(), up.size() * 4, hipMemcpyHostToDevice, stream));
			HIP_TRY(hipStreamSynchronize(stream)); // (`up` is pageable: the copy has left it before it goes)
		}
		l.lists = d_xf_lists.p;
		FilteredScoreArgs m;
		m.sp = view().sp;
		m.queries = b.d_queries;
		m.q_stride = b.q_stride, m.dim = (uint32_t)dim;
		m.order = d_xf_tables.p + at_order;
		m.lists = d_xf_lists.p;
		m.chunk_stride = (uint32_t)CH;
		m.scores = d_scores.p;
		const uint32_t m_lds = qt * V * 16;
		const void *m_fn = metric == 0   ? reinterpret_cast<const void *>(k_exact_filtered_scores<0>)
		                   : metric == 1 ? reinterpret_cast<const void *>(k_exact_filtered_scores<1>)
		                                 : reinterpret_cast<const void *>(k_exact_filtered_scores<2>);
		HIP_TRY(hipFuncSetAttribute(m_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<uint32_t>(m_lds, 64 * 1024)));
		SelectListsArgs s;
		s.scores = d_scores.p;
		s.chunk_stride = (uint32_t)CH;
		s.KP = (uint32_t)KP;
		s.offset = d_xf_tables.p + at_offset, s.length = d_xf_tables.p + at_length, s.lists = d_xf_lists.p;
		s.best_s = d_best_s.p, s.best_i = d_best_i.p;
		for (const ExactFilterPass &pass : plan.passes) {
			const uint32_t n_tiles = pass.tile_end - pass.tile_begin;
			if (!n_tiles)
				continue; // (none of its groups admits a row)
			l.u_begin = pass.group_begin, l.u_end = pass.group_end;
			g.launch_scatter(l, stream);
			m.tiles = reinterpret_cast<const ExactFilterTile *>(d_xf_tables.p + at_tiles) + pass.tile_begin;
			s.query_begin = pass.query_begin;
			for (uint64_t p0 = 0; p0 < pass.longest; p0 += CH) {
				// the launches per pass follow the longest list, never the number of groups: a workgroup column per tile
				const uint64_t cols = std::min<uint64_t>(CH, pass.longest - p0), rows_per_wave_pass = 64u >> logG;
				const uint64_t waves = (cols + rows_per_wave_pass - 1) / rows_per_wave_pass;
				const uint64_t per_tile = std::max<uint64_t>(1, (16ull * n_cus + n_tiles - 1) / n_tiles);
				const dim3 grid((uint32_t)std::min<uint64_t>((waves + 3) / 4, per_tile), n_tiles);
				m.pos_begin = s.pos_begin = (uint32_t)p0;
				if (metric == 0)
					hipLaunchKernelGGL(k_exact_filtered_scores<0>, grid, dim3(256), m_lds, stream, m);
				else if (metric == 1)
					hipLaunchKernelGGL(k_exact_filtered_scores<1>, grid, dim3(256), m_lds, stream, m);
				else
					hipLaunchKernelGGL(k_exact_filtered_scores<2>, grid, dim3(256), m_lds, stream, m);
				hipLaunchKernelGGL(k_exact_select_lists, dim3(pass.query_end - pass.query_begin), dim3(SEL_THREADS), 0, stream, s);
			}
		}
		// the running lists hold slots; row t of them answers query order[t].  A query of an unknown group, of a group that
		// admits nothing, or of an empty index still has its empty list: count 0, cells -1 / +inf.
		RerankArgs r;
		r.gv = view();
		r.queries = b.d_queries;
		r.q_stride = b.q_stride;
		r.n_queries = (uint32_t)nq;
		r.k = (uint32_t)k;
		r.KP = (uint32_t)KP;
		r.best_i = d_best_i.p;
		r.out_keys = out.keys;
		r.out_d = out.dist;
		r.out_count = out.count;
		r.best_s = nullptr, r.norm_ext = nullptr, r.certified = nullptr;
		r.query_map = d_xf_tables.p + at_order;
		const uint32_t lds = align16(V * 16) + 2 * align16((uint32_t)KP * 4);
		launch_by_metric<RerankArgs>(launch_rerank<0>, launch_rerank<1>, launch_rerank<2>, r, launch_cfg((uint32_t)nq, lds, 64));
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(ev[1], stream));
		HIP_TRY(hipStreamSynchronize(stream));
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
		{
			std::lock_guard<std::mutex> lk(stats_mu);
			timing[0] = ms;
		}
		return VSS_OK;
	}

	// the host-pointer form: only the bitmaps are staged, because the plan reads the group numbers on the host
	int exact_filtered_host(const HostCall &hc, const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of) {
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return stage_group_table(c, FilterGroupBatch {allowed, nullptr, n_groups}, n_bits, hc.nq); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &) {
			    return exact_filtered_launch(
			        b, GroupedRows::bitmaps(c.d_group_filter.p, n_groups, n_bits, HostWords(group_of), DeviceWords(nullptr)), out);
		    });
	}

	// ------------------------------------------------------------------ filtered search, routed per group (filter_route.h)
	// One count pass over every group in use feeds the rule and the exact plan; the exact-routed queries are answered straight
	// into the caller's cells by the exact step over lists of exact-routed groups only; the graph-routed ones are gathered into
	// a compact batch of context b.slot, walked by one ordinary search launch and scattered back.  `route` (HOST) is filled here.
	int filtered_auto(const DeviceBatch &b, const GroupedRows &g, uint64_t route_c, const DeviceAnswers &out, std::vector<uint8_t> &route) {
		const uint64_t nq = b.nq, k = b.k;
		const uint64_t limit = filter_route_limit(k, b.ef, efs), C = route_c ? route_c : FILTER_ROUTE_C, L = count - tombstones;
		SearchCtx &c = context(b.slot);
		FilterRoutePlan rp;
		{
			std::lock_guard<std::mutex> exact_lock(exact_mu);
			last_exact_fallbacks = 0;
			std::fill(last_exact_filtered, last_exact_filtered + 4, 0);
			std::fill(last_filter_route, last_filter_route + 8, 0);
			ExactFilterPlan all;
			exact_filter_order(g.group_of, nq, g.n_groups, all);
			std::vector<uint32_t> lengths;
			if (const int rc = exact_filtered_count(all, nq, 2, g, lengths))
				return rc;
			filter_route_partition(all, lengths.data(), g.group_of, nq, L, limit, C, route_c ? 0 : FILTER_ROUTE_MIN_WALK, rp);
			const uint64_t nu = all.groups.size(), nx = rp.exact.groups.size();
			if (!rp.exact.order.empty()) {
				uint32_t *taken_counts = nx == nu ? nullptr : d_xf_counts.p; // (nullptr: the count pass ran over these very groups)
				const uint32_t n_blocks = (uint32_t)((count + FL_WAVE_SLOTS - 1) / FL_WAVE_SLOTS);
				if (nx != nu && n_blocks) {
					// the exact-routed groups' rows of counts, made consecutive behind the nu rows of the count pass; which rows:
					// behind the groups of the count pass's table, whose totals have been read
					taken_counts = d_xf_counts.p + nu * n_blocks;
					uint32_t *d_rows = d_xf_tables.p + ExactFilterTables(nu, nq, g.group_cells()).at_totals;
					HIP_TRY(hipMemcpyAsync(d_rows, rp.exact_rows.data(), nx * 4, hipMemcpyHostToDevice, stream));
					const dim3 grid(std::min<uint32_t>((n_blocks + 255) / 256, 64), (uint32_t)std::min<uint64_t>(nx, 65535));
					hipLaunchKernelGGL(k_route_take_rows, grid, dim3(256), 0, stream, d_xf_counts.p, d_rows, (uint32_t)nx, n_blocks,
					                   taken_counts);
					HIP_TRY(hipStreamSynchronize(stream)); // (the score step rewrites d_xf_tables)
				}
				if (const int rc = exact_filtered_score(rp.exact, rp.exact_lengths, taken_counts, b, g, out))
					return rc;
			}
			last_filter_route[0] = rp.graph_queries.size(), last_filter_route[1] = rp.exact.order.size();
			last_filter_route[2] = rp.n_graph_groups, last_filter_route[3] = rp.n_exact_groups;
			last_filter_route[4] = L, last_filter_route[5] = C, last_filter_route[6] = limit;
		}
		route = rp.route;
		const uint64_t ng = rp.graph_queries.size(), n_unknown = rp.unknown_queries.size();
		if (!ng) { // no walk: the search counters describe none
			std::lock_guard<std::mutex> lk(stats_mu);
			std::fill(last_stats, last_stats + 4, 0);
			std::fill(last_shape, last_shape + 8, 0);
			std::fill(last_prescore, last_prescore + 4, 0);
			last_prescore_descent[0] = last_prescore_descent[1] = 0;
		}
		if (!ng && !n_unknown)
			return VSS_OK;
		std::unique_lock<std::mutex> route_lock(route_mu, std::defer_lock);
		if (b.slot == 0)
			route_lock.lock();
		if (!c.d_route_map.try_grow(ng + n_unknown) || !c.d_route_q.try_grow(std::max<uint64_t>(ng * dim, 1)) ||
		    !c.d_route_group.try_grow(std::max<uint64_t>(ng * g.group_cells(), 1)) || !c.d_route_keys.try_grow(std::max<uint64_t>(ng * k, 1)) ||
		    !c.d_route_d.try_grow(std::max<uint64_t>(ng * k, 1)) || !c.d_route_count.try_grow(std::max<uint64_t>(ng, 1)))
			return fail("routed filtered search: no device memory for a compact batch of %llu queries", (unsigned long long)ng);
		if (n_unknown) {
			HIP_TRY(hipMemcpyAsync(c.d_route_map.p + ng, rp.unknown_queries.data(), n_unknown * 4, hipMemcpyHostToDevice, c.stream));
			hipLaunchKernelGGL(k_route_blank, dim3((uint32_t)((n_unknown + 3) / 4)), dim3(256), 0, c.stream, c.d_route_map.p + ng,
			                   (uint32_t)n_unknown, (uint32_t)k, out.keys, out.dist, out.count);
		}
		if (ng) {
			HIP_TRY(hipMemcpyAsync(c.d_route_map.p, rp.graph_queries.data(), ng * 4, hipMemcpyHostToDevice, c.stream));
			RouteGatherArgs ga;
			ga.queries = b.d_queries, ga.group_of = g.d_group_of, ga.map = c.d_route_map.p;
			ga.n = (uint32_t)ng, ga.q_stride = (uint32_t)dim;
			ga.vec4 = dim % 4 == 0 && reinterpret_cast<uintptr_t>(b.d_queries) % 16 == 0 && reinterpret_cast<uintptr_t>(c.d_route_q.p) % 16 == 0;
			ga.out_queries = c.d_route_q.p, ga.out_group_of = c.d_route_group.p;
			hipLaunchKernelGGL(k_route_gather, dim3((uint32_t)((ng + 3) / 4)), dim3(256), 0, c.stream, ga);
			// (a range's upper ends, behind the ng lower ones; a set's whole rows)
			if (const GroupedRows::WalkWords w = g.more_walk_words(ng); w.words) {
				const dim3 grid((uint32_t)((ng * w.per + 255) / 256));
				void (*const column)(const uint32_t *, const uint32_t *, uint32_t, uint32_t *) = k_route_gather_words;
				void (*const matrix)(const uint32_t *, const uint32_t *, uint32_t, uint32_t, uint32_t *) = k_route_gather_words;
				if (w.per == 1) // (the kernel of the call by label range, as it was)
					hipLaunchKernelGGL(column, grid, dim3(256), 0, c.stream, w.words, c.d_route_map.p, (uint32_t)ng, c.d_route_group.p + w.at);
				else
					hipLaunchKernelGGL(matrix, grid, dim3(256), 0, c.stream, w.words, c.d_route_map.p, (uint32_t)ng, w.per,
					                   c.d_route_group.p + w.at);
			}
			HIP_TRY(hipGetLastError());
			SearchRequest r = request(b.slot, &c.d_route_q.p, 1, ng, k, b.ef, &c.d_route_keys.p, &c.d_route_d.p, &c.d_route_count.p);
			r.predicate = g.walk_predicate(c.d_route_group.p, ng);
			if (const int rc = search_launch(r))
				return rc;
			RouteScatterArgs s;
			s.map = c.d_route_map.p, s.n = (uint32_t)ng, s.k = (uint32_t)k;
			s.keys = c.d_route_keys.p, s.dist = c.d_route_d.p, s.count = c.d_route_count.p;
			s.out_keys = out.keys, s.out_dist = out.dist, s.out_count = out.count;
			hipLaunchKernelGGL(k_route_scatter, dim3((uint32_t)((ng + 3) / 4)), dim3(256), 0, c.stream, s);
		}
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(c.stream));
		return VSS_OK;
	}

	// the host-pointer form: the whole table is staged, and the leased context also carries the walk
	int filtered_auto_host(const HostCall &hc, const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of,
	                       uint64_t route_c) {
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return stage_group_table(c, FilterGroupBatch {allowed, group_of, n_groups}, n_bits, hc.nq); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &route) {
			    const DeviceWords d_group_of(group_of ? c.d_group_of.p : nullptr);
			    return filtered_auto(b, GroupedRows::bitmaps(c.d_group_filter.p, n_groups, n_bits, HostWords(group_of), d_group_of), route_c,
			                         out, route);
		    });
	}

	// ------------------------------------------------------------------ search by label (label_filter.h)
	// The routed call over the table label_groups() makes of `want`: group g = the rows labelled values[g].  d_want: the same
	// values for the walk of the graph-routed queries; nullptr asks for the exact scan of every query, which has no walk to read
	// them.  No bitmap exists anywhere; the plans, the rule and the counters are those of the bitmap calls.
	int by_label_launch(const DeviceBatch &b, HostWords want, DeviceWords d_want, uint64_t route_c, const DeviceAnswers &out,
	                    std::vector<uint8_t> &route) {
		std::vector<uint32_t> values, group_of;
		label_groups(want.p, b.nq, values, group_of);
		const GroupedRows g = GroupedRows::labels(values, d_labels.p, labelled_rows, HostWords(group_of.data()), d_want);
		if (!d_want.p) {
			route.assign(b.nq, FILTER_ROUTE_EXACT);
			return exact_filtered_launch(b, g, out);
		}
		return filtered_auto(b, g, route_c, out, route);
	}

	// the host-pointer form of those two: the exact scan stages no wanted labels
	int by_label_host(const HostCall &hc, bool exact, const uint32_t *want, uint64_t route_c) {
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return exact ? (int)VSS_OK : stage_wanted_labels(c, want, hc.nq); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &route) {
			    return by_label_launch(b, HostWords(want), DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, out, route);
		    });
	}

	// ------------------------------------------------------------------ search by label range (label_filter.h)
	// The same over the table label_range_groups() makes of (lo, hi): group g = the rows whose label lies within pairs[g].  d_lo /
	// d_hi: the ends for the walk of the graph-routed queries; nullptr asks for the exact scan of every query.
	int by_range_launch(const DeviceBatch &b, HostWords lo, HostWords hi, DeviceWords d_lo, DeviceWords d_hi, uint64_t route_c,
	                    const DeviceAnswers &out, std::vector<uint8_t> &route) {
		std::vector<LabelRange> pairs;
		std::vector<uint32_t> group_of;
		label_range_groups(lo.p, hi.p, b.nq, pairs, group_of);
		const GroupedRows g = GroupedRows::ranges(pairs, d_labels.p, labelled_rows, HostWords(group_of.data()), d_lo, d_hi);
		if (!d_lo.p) {
			route.assign(b.nq, FILTER_ROUTE_EXACT);
			return exact_filtered_launch(b, g, out);
		}
		return filtered_auto(b, g, route_c, out, route);
	}

	// the host-pointer form of those two: the exact scan stages no ends
	int by_range_host(const HostCall &hc, bool exact, const uint32_t *lo, const uint32_t *hi, uint64_t route_c) {
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return exact ? (int)VSS_OK : stage_label_ranges(c, lo, hi, hc.nq); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &route) {
			    return by_range_launch(b, HostWords(lo), HostWords(hi), DeviceWords(exact ? nullptr : c.d_group_of.p),
			                           DeviceWords(exact ? nullptr : c.d_group_of.p + hc.nq), route_c, out, route);
		    });
	}

	// ------------------------------------------------------------------ search by label set (label_filter.h)
	// The same over the table label_set_groups() makes of `sets`: group g = the rows whose label is a word of rows[g].  d_sets: the
	// matrix for the walk of the graph-routed queries; nullptr asks for the exact scan of every query.
	int by_set_launch(const DeviceBatch &b, HostWords sets, uint32_t width, DeviceWords d_sets, uint64_t route_c, const DeviceAnswers &out,
	                  std::vector<uint8_t> &route) {
		std::vector<uint32_t> rows, group_of;
		label_set_groups(sets.p, b.nq, width, rows, group_of);
		const GroupedRows g = GroupedRows::sets(rows, width, d_labels.p, labelled_rows, HostWords(group_of.data()), d_sets);
		if (!d_sets.p) {
			route.assign(b.nq, FILTER_ROUTE_EXACT);
			return exact_filtered_launch(b, g, out);
		}
		return filtered_auto(b, g, route_c, out, route);
	}

	// the host-pointer form of those two: the exact scan stages no sets
	int by_set_host(const HostCall &hc, bool exact, const uint32_t *sets, uint32_t width, uint64_t route_c) {
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return exact ? (int)VSS_OK : stage_label_sets(c, sets, width, hc.nq); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &route) {
			    return by_set_launch(b, HostWords(sets), width, DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, out, route);
		    });
	}

	// ------------------------------------------------------------------ search by label box (label_filter.h)
	// The same over the table label_box_groups() makes of `boxes` (nq x 2m, HOST): group g = the rows inside rows[g] in every named
	// column.  d_boxes: the matrix for the walk of the graph-routed queries; nullptr asks for the exact scan of every query.
	int by_box_launch(const DeviceBatch &b, HostWords boxes, const LabelBoxColumns &box, DeviceWords d_boxes, uint64_t route_c,
	                  const DeviceAnswers &out, std::vector<uint8_t> &route) {
		std::vector<uint32_t> rows, group_of;
		label_box_groups(boxes.p, b.nq, box.m, rows, group_of);
		const GroupedRows g = GroupedRows::boxes(rows, box, HostWords(group_of.data()), d_boxes);
		if (!d_boxes.p) {
			route.assign(b.nq, FILTER_ROUTE_EXACT);
			return exact_filtered_launch(b, g, out);
		}
		return filtered_auto(b, g, route_c, out, route);
	}

	// the host-pointer form of those two: the exact scan stages no boxes
	int by_box_host(const HostCall &hc, bool exact, const uint32_t *boxes, const LabelBoxColumns &box, uint64_t route_c) {
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return exact ? (int)VSS_OK : stage_label_boxes(c, boxes, box.m, hc.nq); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &route) {
			    return by_box_launch(b, HostWords(boxes), box, DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, out, route);
		    });
	}

	// ------------------------------------------------------------------ search by label box64 (label_filter.h)
	// The same with 64-bit ends: `boxes` is nq x 4m words (label_box64_rows), and the named columns may be of either width.
	int by_box64_launch(const DeviceBatch &b, HostWords boxes, const LabelBoxColumns &box, DeviceWords d_boxes, uint64_t route_c,
	                    const DeviceAnswers &out, std::vector<uint8_t> &route) {
		std::vector<uint32_t> rows, group_of;
		label_box64_groups(boxes.p, b.nq, box.m, rows, group_of);
		const GroupedRows g = GroupedRows::boxes64(rows, box, HostWords(group_of.data()), d_boxes);
		if (!d_boxes.p) {
			route.assign(b.nq, FILTER_ROUTE_EXACT);
			return exact_filtered_launch(b, g, out);
		}
		return filtered_auto(b, g, route_c, out, route);
	}

	int by_box64_host(const HostCall &hc, bool exact, const uint32_t *boxes, const LabelBoxColumns &box, uint64_t route_c) {
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return exact ? (int)VSS_OK : stage_label_boxes(c, boxes, box.m, hc.nq, 2); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &route) {
			    return by_box64_launch(b, HostWords(boxes), box, DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, out, route);
		    });
	}

	// ------------------------------------------------------------------ search by label set box (label_filter.h)
	// An IN-list on one column inside a box of ranges: `rows` is nq travelling rows (label_set_box_rows), `box` names the set column
	// first and the range columns after it.
	int by_set_box_launch(const DeviceBatch &b, HostWords rows_in, uint32_t set_width, const LabelBoxColumns &box, DeviceWords d_rows,
	                      uint64_t route_c, const DeviceAnswers &out, std::vector<uint8_t> &route) {
		std::vector<uint32_t> rows, group_of;
		label_set_box_groups(rows_in.p, b.nq, set_width, box.m - 1, rows, group_of);
		const GroupedRows g = GroupedRows::set_boxes(rows, set_width, box, HostWords(group_of.data()), d_rows);
		if (!d_rows.p) {
			route.assign(b.nq, FILTER_ROUTE_EXACT);
			return exact_filtered_launch(b, g, out);
		}
		return filtered_auto(b, g, route_c, out, route);
	}

	int by_set_box_host(const HostCall &hc, bool exact, const uint32_t *rows, uint32_t set_width, const LabelBoxColumns &box, uint64_t route_c) {
		const uint32_t row_words = label_set_box_row_words(set_width, box.m - 1);
		return staged_call(
		    hc, true, [&](SearchCtx &c) { return exact ? (int)VSS_OK : stage_label_set_boxes(c, rows, row_words, hc.nq); },
		    [&](SearchCtx &c, const DeviceBatch &b, const DeviceAnswers &out, std::vector<uint8_t> &route) {
			    return by_set_box_launch(b, HostWords(rows), set_width, box, DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, out, route);
		    });
	}

	// The device forms of these calls: the plans and the rule read a per-query column on the host, so 4 bytes per query come back
	// first (d_words == nullptr: there is no column, and the vector stays empty) ...
	std::vector<uint32_t> words_to_host(const uint32_t *d_words, uint64_t nq) {
		std::vector<uint32_t> words;
		if (d_words) {
			words.resize(nq);
			HIP_TRY(hipMemcpyAsync(words.data(), d_words, nq * 4, hipMemcpyDeviceToHost, stream));
			HIP_TRY(hipStreamSynchronize(stream));
		}
		return words;
	}
	// ... and the route table goes to the caller's DEVICE cells last (d_out_route may be nullptr)
	void route_to_device(const std::vector<uint8_t> &route, uint8_t *d_out_route) {
		if (!d_out_route)
			return;
		HIP_TRY(hipMemcpyAsync(d_out_route, route.data(), route.size(), hipMemcpyHostToDevice, stream));
		HIP_TRY(hipStreamSynchronize(stream));
	}

	// ------------------------------------------------------------------ remove
	void ensure_keymap() {
		if (keymap.ready)
			return;
		keymap.init(count + staged);
		for (uint64_t i = 0; i != count + staged; ++i)
			if (keys_h[i] != VSS_FREE_KEY)
				keymap.put(keys_h[i], (uint32_t)i);
	}

	int remove(const int64_t *rowids, uint64_t n, uint64_t *removed) {
		if (removed)
			*removed = 0;
		if (staged || n_pending)
			return fail("cannot remove while staged rows are unlinked (call vss_build_finalize first)");
		if (refuse_while_probing("vss_remove_batch") != VSS_OK)
			return VSS_ERROR;
		ensure_keymap();
		std::vector<uint32_t> slots;
		for (uint64_t i = 0; i != n; ++i) {
			uint32_t slot;
			if (!keymap.find(rowids[i], slot))
				continue;
			if (!free_slots.reserve(free_slots.size() + 1)) // index_dense.hpp:1239-1240
				return fail("Can't allocate memory for a free-list");
			free_slots.push(slot);
			keymap.erase(rowids[i]);
			keys_h[slot] = VSS_FREE_KEY;
			slots.push_back(slot);
		}
		if (!slots.empty()) { // one upload + one kernel for the whole batch
			d_work_build.ensure(slots.size(), 0, stream);
			HIP_TRY(hipMemcpyAsync(d_work_build.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, stream));
			const uint32_t tb = 256, gb = (uint32_t)std::min<uint64_t>((slots.size() + tb - 1) / tb, 1024);
			hipLaunchKernelGGL(k_mark_removed, dim3(gb), dim3(tb), 0, stream, d_keys.p, d_work_build.p,
			                   (uint32_t)slots.size());
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(stream));
			tombstones += slots.size();
			mutations++;
		}
		if (removed)
			*removed = slots.size();
		return VSS_OK;
	}

	// ------------------------------------------------------------------ stream format (usearch 2.12)
	uint64_t node_bytes(int level) const {
		return 10 + (4 + 4 * M0) + (uint64_t)level * (4 + 4 * M);
	}
	uint64_t serialized_length() const {
		uint64_t n = 8 + count * dim * 4 + 64 + 40;
		for (uint64_t i = 0; i != count; ++i)
			n += node_bytes(levels_h[i]) + 2;
		return n;
	}

	int save(vss_write_cb write, void *ctx) {
		if (staged || n_pending)
			return fail("cannot serialise with staged, unlinked rows (call vss_build_finalize first)");
		const uint64_t stride = (uint64_t)V * 4;
		auto put = [&](const void *p, uint64_t n) -> bool { return n == 0 || write(ctx, p, n) != 0; };
		uint32_t dims[2] = {(uint32_t)count, (uint32_t)(dim * 4)};
		if (!put(dims, 8))
			return fail("Failed to serialize into stream");
		// vectors in slot order, un-padded, in slabs
		{
			const uint64_t slab = std::max<uint64_t>(1, (64ull << 20) / (dim * 4));
			std::vector<float> buf(slab * dim);
			for (uint64_t r0 = 0; r0 < count; r0 += slab) {
				const uint64_t nr = std::min(slab, count - r0);
				HIP_TRY(hipMemcpy2DAsync(buf.data(), dim * 4, d_vectors.p + r0 * stride, stride * 4, dim * 4, nr,
				                         hipMemcpyDeviceToHost, stream));
				HIP_TRY(hipStreamSynchronize(stream));
				if (!put(buf.data(), nr * dim * 4))
					return fail("Failed to serialize into stream");
			}
		}
		uint8_t head[64];
		std::memset(head, 0, 64);
		std::memcpy(head, "usearch", 7);
		uint16_t ver[3] = {2, 12, 0};
		std::memcpy(head + 7, ver, 6);
		head[13] = metric == 0 ? 'e' : metric == 1 ? 'c' : 'i';
		head[14] = 11, head[15] = 20, head[16] = 15;
		uint64_t present = count - tombstones, deleted = tombstones, dimensions = dim;
		std::memcpy(head + 17, &present, 8);
		std::memcpy(head + 25, &deleted, 8);
		std::memcpy(head + 33, &dimensions, 8);
		if (!put(head, 64))
			return fail("Failed to serialize into stream");
		uint64_t gh[5] = {count, M, M0, (uint64_t)(int64_t)(count ? max_level : -1), entry};
		if (!put(gh, 40))
			return fail("Failed to serialize the header into stream");
		std::vector<int16_t> lv(count);
		for (uint64_t i = 0; i != count; ++i)
			lv[i] = levels_h[i];
		if (!put(lv.data(), count * 2))
			return fail("Failed to serialize into stream");
		std::vector<uint32_t> l0(count * M0), lu(n_upper * M);
		HIP_TRY(hipMemcpyAsync(l0.data(), d_links0.p, l0.size() * 4, hipMemcpyDeviceToHost, stream));
		if (n_upper)
			HIP_TRY(hipMemcpyAsync(lu.data(), d_links_up.p, lu.size() * 4, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		std::vector<uint8_t> out;
		out.reserve(1 << 20);
		auto emit_list = [&](const uint32_t *src, uint64_t cap) {
			uint32_t cnt = 0;
			while (cnt < cap && src[cnt] != EMPTY_SLOT)
				cnt++;
			const size_t at = out.size();
			out.resize(at + 4 + 4 * cap, 0);
			std::memcpy(out.data() + at, &cnt, 4);
			std::memcpy(out.data() + at + 4, src, 4 * (size_t)cnt);
		};
		for (uint64_t i = 0; i != count; ++i) {
			const size_t at = out.size();
			out.resize(at + 10);
			std::memcpy(out.data() + at, &keys_h[i], 8);
			std::memcpy(out.data() + at + 8, &lv[i], 2);
			emit_list(l0.data() + i * M0, M0);
			for (int l = 0; l < lv[i]; ++l)
				emit_list(lu.data() + ((uint64_t)upper_off_h[i] + l) * M, M);
			if (out.size() >= (1 << 20) || i + 1 == count) {
				if (!put(out.data(), out.size()))
					return fail("Failed to serialize into stream");
				out.clear();
			}
		}
		return VSS_OK;
	}

	int load(vss_read_cb read, void *ctx) {
		if (refuse_while_probing("vss_load") != VSS_OK)
			return VSS_ERROR;
		auto get = [&](void *p, uint64_t n) -> bool { return n == 0 || read(ctx, p, n) != 0; };
		uint32_t dims[2];
		if (!get(dims, 8))
			return fail("Failed to read 32-bit dimensions of the matrix");
		const uint64_t rows = dims[0], cols = dims[1];
		std::vector<float> vecs(rows * cols / 4);
		if (!get(vecs.data(), rows * cols))
			return fail("Failed to read vectors");
		uint8_t head[64];
		if (!get(head, 64))
			return fail("Failed to read the index ");
		if (std::memcmp(head, "usearch", 7) != 0)
			return fail("Magic header mismatch - the file isn't an index");
		uint16_t ver_major;
		std::memcpy(&ver_major, head + 7, 2);
		if (ver_major != 2)
			return fail("File format may be different, please rebuild");
		if (head[15] != 20)
			return fail("Key type doesn't match, consider rebuilding");
		if (head[16] != 15)
			return fail("Slot type doesn't match, consider rebuilding");
		if (head[14] != 11)
			return fail("Only f32 vectors are supported");
		uint64_t dimensions;
		std::memcpy(&dimensions, head + 33, 8);
		const int m = head[13] == 'e' ? 0 : head[13] == 'c' ? 1 : head[13] == 'i' ? 2 : -1;
		if (m < 0)
			return fail("Unsupported metric kind in stream");
		uint64_t gh[5];
		if (!get(gh, 40))
			return fail("Failed to pull the header from the stream");
		if (rows && cols != dimensions * 4)
			return fail("Vector size in stream doesn't match its dimensions");
		// Parse and validate the whole stream into temporaries first: a corrupt or truncated stream must leave the handle
		// as it was, and every slot number the kernels will follow must be in range.
		const uint64_t sM = gh[1], sM0 = gh[2];
		if (rows != gh[0])
			return fail("Index size and the number of vectors doesn't match");
		if (rows && (sM < 2 || sM0 < sM))
			return fail("Corrupt connectivity in stream");
		if (rows >= 0x7FFFFFFFull)
			return fail("capacity above 2^31-1 slots is not supported");
		std::vector<int16_t> lv(rows);
		std::vector<uint8_t> t_levels(rows);
		std::vector<uint32_t> t_off(rows), t_owner, l0, lu;
		std::vector<int64_t> t_keys(rows);
		std::vector<uint32_t> named_by(rows, EMPTY_SLOT); // last list (numbered as read) that named each slot
		uint32_t lists_read = 0;
		bool t_repeat = false;
		uint64_t upper = 0, t_tomb = 0;
		if (rows) {
			if (!get(lv.data(), rows * 2))
				return fail("Failed to pull nodes levels from the stream");
			for (uint64_t i = 0; i != rows; ++i) {
				if (lv[i] < 0 || lv[i] > 255)
					return fail("Corrupt level in stream");
				t_levels[i] = (uint8_t)lv[i];
				t_off[i] = (uint32_t)upper;
				upper += lv[i];
			}
			const int64_t s_max_level = (int64_t)gh[3];
			if (gh[4] >= rows || s_max_level != lv[gh[4]])
				return fail("Corrupt entry point in stream");
			for (uint64_t i = 0; i != rows; ++i)
				if (lv[i] > s_max_level)
					return fail("Corrupt level in stream");
			t_owner.resize(upper);
			l0.assign(rows * sM0, EMPTY_SLOT);
			lu.assign(upper * sM, EMPTY_SLOT);
			std::vector<uint8_t> tape;
			for (uint64_t i = 0; i != rows; ++i) {
				tape.resize(10 + (4 + 4 * sM0) + (uint64_t)lv[i] * (4 + 4 * sM));
				if (!get(tape.data(), tape.size()))
					return fail("Failed to pull nodes from the stream");
				std::memcpy(&t_keys[i], tape.data(), 8);
				int16_t record_level;
				std::memcpy(&record_level, tape.data() + 8, 2);
				if (record_level != lv[i])
					return fail("Corrupt level in stream");
				t_tomb += t_keys[i] == VSS_FREE_KEY;
				const uint8_t *p = tape.data() + 10;
				for (int l = 0; l <= lv[i]; ++l) {
					const uint64_t cap = l ? sM : sM0;
					uint32_t cnt;
					std::memcpy(&cnt, p, 4);
					if (cnt > cap)
						return fail("Corrupt neighbour count in stream");
					uint32_t *dst = l ? lu.data() + ((uint64_t)t_off[i] + l - 1) * sM : l0.data() + i * sM0;
					std::memcpy(dst, p + 4, 4 * (size_t)cnt);
					for (uint32_t j = 0; j != cnt; ++j) {
						if (dst[j] >= rows || lv[dst[j]] < l)
							return fail("Corrupt neighbour slot in stream");
						t_repeat |= named_by[dst[j]] == lists_read;
						named_by[dst[j]] = lists_read;
					}
					lists_read++;
					if (l)
						t_owner[t_off[i] + l - 1] = (uint32_t)i;
					p += 4 + 4 * cap;
				}
			}
		}
		// adopt the stream's shape (usearch load_from_stream resets and re-reserves: index.hpp:3172-3186)
		release_graph_only();
		reset_graph();
		configure(dimensions, m, sM, sM0);
		if (!rows)
			return VSS_OK;
		int rc = reserve(rows, 1);
		if (rc != VSS_OK)
			return rc;
		std::memcpy(levels_h.data(), t_levels.data(), rows);
		std::memcpy(upper_off_h.data(), t_off.data(), rows * 4);
		std::memcpy(keys_h.data(), t_keys.data(), rows * 8);
		ensure_upper(upper);
		list_owner_h.swap(t_owner);
		tombstones = t_tomb;
		lists_may_repeat = t_repeat;
		const uint64_t stride = (uint64_t)V * 4;
		codes_stale.mark_all();
		HIP_TRY(hipMemcpy2DAsync(d_vectors.p, stride * 4, vecs.data(), dim * 4, dim * 4, rows, hipMemcpyHostToDevice,
		                         stream));
		HIP_TRY(hipMemcpyAsync(d_links0.p, l0.data(), l0.size() * 4, hipMemcpyHostToDevice, stream));
		if (upper) {
			HIP_TRY(hipMemcpyAsync(d_links_up.p, lu.data(), lu.size() * 4, hipMemcpyHostToDevice, stream));
			HIP_TRY(hipMemcpyAsync(d_list_owner.p, list_owner_h.data(), upper * 4, hipMemcpyHostToDevice, stream));
		}
		HIP_TRY(hipMemcpyAsync(d_levels.p, levels_h.data(), rows, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipMemcpyAsync(d_upper_off.p, upper_off_h.data(), rows * 4, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipMemcpyAsync(d_keys.p, keys_h.data(), rows * 8, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		n_upper = upper;
		count = rows;
		max_level = (int)(int16_t)gh[3];
		entry = (uint32_t)gh[4];
		if (tombstones) { // reindex_keys_ rebuilds the free list in slot order (index_dense.hpp:1901-1930)
			free_slots.clear();
			free_slots.reserve(tombstones);
			for (uint64_t i = 0; i != rows; ++i)
				if (keys_h[i] == VSS_FREE_KEY)
					free_slots.push((uint32_t)i);
		}
		mutations++;
		return VSS_OK;
	}

	void release_graph_only() {
		d_vectors.free(), d_links0.free(), d_links_up.free(), d_upper_off.free(), d_list_owner.free();
		d_levels.free(), d_keys.free(), d_list_count.free(), d_list_offset.free(), d_row_norm2.free();
		free_codes();
	}

	void configure(uint64_t dim_, int metric_, uint64_t M_, uint64_t M0_) {
		dim = dim_;
		metric = metric_;
		M = M_;
		M0 = M0_;
		V = (uint32_t)((dim + 3) / 4);
		G = (uint32_t)std::min<size_t>(64, ceil_pow2(V));
		logG = log2u(G);
		inv_log_m = inverse_log_connectivity(M);
	}

	// ------------------------------------------------------------------ compact (drops tombstones)
	int compact(bool reorder);
	bool last_compact_reordered = false;
	bool reorder_after_build = false;

	void level_stats(uint64_t level, uint64_t *out4) {
		// usearch index.hpp:3010-3027 (including its inverted max_edges connectivity)
		uint64_t nodes = 0, edges = 0;
		std::vector<uint32_t> lists;
		if (level == 0) {
			lists.resize(count * M0);
			if (count)
				HIP_TRY(hipMemcpy(lists.data(), d_links0.p, lists.size() * 4, hipMemcpyDeviceToHost));
			for (uint64_t i = 0; i != count; ++i) {
				nodes++;
				for (uint64_t j = 0; j != M0 && lists[i * M0 + j] != EMPTY_SLOT; ++j)
					edges++;
			}
		} else {
			lists.resize(n_upper * M);
			if (n_upper)
				HIP_TRY(hipMemcpy(lists.data(), d_links_up.p, lists.size() * 4, hipMemcpyDeviceToHost));
			for (uint64_t i = 0; i != count; ++i) {
				if (levels_h[i] < level)
					continue;
				nodes++;
				const uint32_t *lp = lists.data() + ((uint64_t)upper_off_h[i] + level - 1) * M;
				for (uint64_t j = 0; j != M && lp[j] != EMPTY_SLOT; ++j)
					edges++;
			}
		}
		out4[0] = nodes;
		out4[1] = edges;
		out4[2] = nodes * (level ? M0 : M);
		out4[3] = nodes * (10 + 4 + 4 * (level ? M : M0));
	}
};

// ---------------------------------------------------------------------------------------------------------
// The launch gate is per DEVICE, not per index: launches of different indexes on one GPU (row-range shards placed on the
// same device, host/sharded_index.hpp) compete for the same compute units exactly like launches of one index.
// g_gate[device] names the context of the most recent gated launch.  Every device slot has a mutex of its own, held while
// waiting — which also keeps the named index alive: vss_destroy clears its entry under the same mutex — so a wait on one
// GPU never delays launches (or vss_destroy) on another one of a process that drives several.
// ---------------------------------------------------------------------------------------------------------
namespace {
struct GateEntry {
	vss_index *owner = nullptr;
	int ctx = -1;
};
struct DeviceGate {
	std::mutex mu;
	GateEntry last;
};
DeviceGate g_gate[64];
} // namespace

void vss_index::wait_for_drain_of_previous_launch(int slot) {
	DeviceGate &dg = g_gate[(unsigned)device % 64];
	std::lock_guard<std::mutex> lk(dg.mu);
	GateEntry &g = dg.last;
	const GateEntry prev = g;
	g.owner = this, g.ctx = slot;
	if (!search_gating || !prev.owner || (prev.owner == this && prev.ctx == slot))
		return;
	SearchCtx &pc = prev.owner->ctx[prev.ctx];
	if (!pc.h_queue || !pc.ev1)
		return;
	volatile uint32_t *drained = pc.h_queue + 2;
	while (*drained == 0) {
		if (hipEventQuery(pc.ev1) != hipErrorNotReady)
			break; // finished (or never started): nothing to wait for
		std::this_thread::yield();
	}
	(void)hipGetLastError(); // hipErrorNotReady is an answer, not an error to be found by the next launch check
}

// ---------------------------------------------------------------------------------------------------------
// compact.  Two things happen, both on the device:
//   * tombstoned nodes are dropped and links to them removed, the remaining links keep their order (the DOCUMENTED
//     behaviour of PRAGMA hnsw_compact_index, reference README.md:69; usearch's own compact keeps them);
//   * reorder = true (vss_compact): the survivors are renumbered in the reference's compaction order — (level descending,
//     cluster ascending), cluster = the node the greedy descent from the entry lands on above level 0 (index_gt::compact,
//     index.hpp:3405-3494) — with the old slot as the final key (the reference's std::sort leaves that to the library).
//     Nodes of one cluster become neighbours in memory: the rows a search touches lie in a few contiguous runs.
//     reorder = false (vss_compact_ex(.., 0), and the fall-back when a second vector buffer cannot be allocated): the
//     survivors keep their relative order.
// The host derives the slot maps from its key / level mirrors and the cluster array (O(n) counting sorts) and uploads them;
// lists, keys, levels and the vector rows move on the device (k_node_clusters, k_compact_links, k_compact_rows).  Every
// new array is built aside and swapped in only when everything succeeded.  Mirrored by the oracle's compact_dropping() /
// compact_reordering().
// ---------------------------------------------------------------------------------------------------------
int vss_index::compact(bool reorder) {
	if (staged || n_pending)
		return fail("cannot compact with staged, unlinked rows");
	if (refuse_while_probing("vss_compact") != VSS_OK)
		return VSS_ERROR;
	last_compact_reordered = false; // true only once reordered arrays have been swapped in (vss_compact_ex's out_reordered)
	if (!count || (!tombstones && !reorder))
		return VSS_OK;
	const uint64_t stride = (uint64_t)V * 4;
	const uint64_t live = count - tombstones;
	// The rows are gathered into a second buffer that replaces the old one on success.  Without one (not enough free HBM) a
	// permutation is impossible: the compaction then only prunes, moving the rows down in place.
	DevBuf<float> n_vectors;
	struct FreeOnExit { // whatever way this function is left (the host-side sorts below allocate and may throw): no HBM stays behind
		DevBuf<float> &b;
		~FreeOnExit() {
			b.free();
		}
	} n_vectors_guard {n_vectors};
	{
		float *np = nullptr;
		const char *in_place = getenv("VSS_COMPACT_IN_PLACE"); // tests: take the no-second-buffer path although HBM is free
		if (!(in_place && atoi(in_place)) && hipMalloc(&np, d_vectors.n * sizeof(float)) == hipSuccess) {
			n_vectors.p = np, n_vectors.n = d_vectors.n;
		} else {
			(void)hipGetLastError();
			reorder = false;
			if (!tombstones)
				return VSS_OK;
		}
	}
	const bool fresh_rows = n_vectors.p != nullptr;
	codes_stale.mark_all(); // rows move (in place, or into the fresh buffer that is swapped in): every code is stale from here on
	// ---- the order of the survivors: src_of[new slot] = old slot
	std::vector<uint32_t> src_of;
	src_of.reserve(live);
	if (!reorder) {
		for (uint64_t i = 0; i != count; ++i)
			if (keys_h[i] != VSS_FREE_KEY)
				src_of.push_back((uint32_t)i);
	} else {
		std::vector<uint32_t> cluster(count);
		DevBuf<uint32_t> d_cluster;
		try {
			d_cluster.ensure(count, 0, stream);
			d_work_stats.ensure(4, 0, stream, 0);
			ClusterArgs ca;
			ca.gv = view();
			ca.count = (uint32_t)count;
			ca.entry = entry;
			ca.max_level = max_level;
			ca.list_cap_max = list_cap_max();
			ca.cluster = d_cluster.p;
			ca.work_stats = nullptr;
			const uint32_t lds = wave_lds_bytes(4, V, ca.list_cap_max, 16);
			launch_by_metric<ClusterArgs>(launch_clusters<0>, launch_clusters<1>, launch_clusters<2>, ca,
			                              launch_cfg((uint32_t)std::min<uint64_t>(count, (uint64_t)n_cus * 64), lds, 64));
			HIP_TRY(hipMemcpyAsync(cluster.data(), d_cluster.p, count * 4, hipMemcpyDeviceToHost, stream));
			HIP_TRY(hipStreamSynchronize(stream));
		} catch (...) {
			d_cluster.free(), n_vectors.free();
			throw;
		}
		d_cluster.free();
		// stable counting sorts, least significant key first: by cluster (ascending), then by level (descending); the input
		// is in slot order, so equal (level, cluster) keep ascending old slots
		std::vector<uint32_t> by_cluster(live), start(count + 1, 0);
		for (uint64_t i = 0; i != count; ++i)
			if (keys_h[i] != VSS_FREE_KEY)
				start[cluster[i] + 1]++;
		for (uint64_t c = 0; c != count; ++c)
			start[c + 1] += start[c];
		for (uint64_t i = 0; i != count; ++i)
			if (keys_h[i] != VSS_FREE_KEY)
				by_cluster[start[cluster[i]]++] = (uint32_t)i;
		uint64_t lstart[257] = {0};
		for (uint32_t sidx : by_cluster)
			lstart[(255 - levels_h[sidx]) + 1]++;
		for (int b = 0; b != 256; ++b)
			lstart[b + 1] += lstart[b];
		src_of.resize(live);
		for (uint32_t sidx : by_cluster)
			src_of[lstart[255 - levels_h[sidx]]++] = sidx;
	}
	std::vector<uint32_t> remap(count, EMPTY_SLOT), noff(live);
	uint64_t nup = 0, first_moved = live;
	for (uint64_t t = 0; t != live; ++t) {
		remap[src_of[t]] = (uint32_t)t;
		noff[t] = (uint32_t)nup;
		nup += levels_h[src_of[t]];
		if (src_of[t] != t)
			first_moved = std::min(first_moved, t);
	}
	// new entry point: the old one if it survives, else the surviving node of the highest level (lowest new slot among
	// equals: with the reordering that is new slot 0)
	int nml = -1;
	uint32_t nentry = 0;
	if (remap[entry] != EMPTY_SLOT) {
		nml = max_level;
		nentry = remap[entry];
	} else {
		for (uint64_t t = 0; t != live; ++t)
			if ((int)levels_h[src_of[t]] > nml)
				nml = levels_h[src_of[t]], nentry = (uint32_t)t;
	}
	DevBuf<uint32_t> d_remap, d_src, d_noff, n_links0, n_links_up, n_owner, n_upper_off;
	DevBuf<uint8_t> n_levels;
	DevBuf<int64_t> n_keys;
	DevBuf<float> staging;
	auto drop_scratch = [&] {
		d_remap.free(), d_src.free(), d_noff.free(), n_links0.free(), n_links_up.free(), n_owner.free(), n_upper_off.free();
		n_levels.free(), n_keys.free(), staging.free(), n_vectors.free();
	};
	try {
		d_remap.ensure(count, 0, stream), d_src.ensure(std::max<uint64_t>(live, 1), 0, stream);
		d_noff.ensure(std::max<uint64_t>(live, 1), 0, stream);
		HIP_TRY(hipMemcpyAsync(d_remap.p, remap.data(), count * 4, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipMemcpyAsync(d_src.p, src_of.data(), live * 4, hipMemcpyHostToDevice, stream));
		HIP_TRY(hipMemcpyAsync(d_noff.p, noff.data(), live * 4, hipMemcpyHostToDevice, stream));
		n_links0.ensure(d_links0.n, 0, stream, 0xFF);
		n_links_up.ensure(d_links_up.n, 0, stream, 0xFF);
		n_owner.ensure(d_list_owner.n, 0, stream, 0);
		n_upper_off.ensure(d_upper_off.n, 0, stream, 0);
		n_levels.ensure(d_levels.n, 0, stream, 0);
		n_keys.ensure(d_keys.n, 0, stream, 0);
		HIP_TRY(hipMemcpyAsync(n_upper_off.p, noff.data(), live * 4, hipMemcpyHostToDevice, stream));
		CompactArgs a;
		a.src_of = d_src.p, a.remap = d_remap.p, a.live = (uint32_t)live;
		a.V = V, a.M = (uint32_t)M, a.M0 = (uint32_t)M0;
		a.vectors = reinterpret_cast<const float4 *>(d_vectors.p);
		a.links0 = d_links0.p, a.links_up = d_links_up.p, a.upper_off = d_upper_off.p;
		a.levels = d_levels.p, a.keys = d_keys.p;
		a.links0_new = n_links0.p, a.links_up_new = n_links_up.p, a.list_owner_new = n_owner.p;
		a.upper_off_new = d_noff.p, a.levels_new = n_levels.p, a.keys_new = n_keys.p;
		a.staging = nullptr;
		if (live) {
			const uint32_t gl = (uint32_t)std::min<uint64_t>((live + 3) / 4, 16384);
			hipLaunchKernelGGL(k_compact_links, dim3(gl), dim3(256), 0, stream, a);
			HIP_TRY(hipGetLastError());
		}
		if (fresh_rows) { // every surviving row is gathered into the fresh buffer (a permutation when reordering)
			HIP_TRY(hipMemsetAsync(n_vectors.p + live * stride, 0, (n_vectors.n - live * stride) * sizeof(float), stream));
			a.staging = reinterpret_cast<float4 *>(n_vectors.p);
			for (uint64_t t0 = 0; t0 < live; t0 += 1u << 30) { // (k_compact_rows numbers rows with 32 bits)
				const uint64_t n = std::min<uint64_t>(1u << 30, live - t0);
				a.staging = reinterpret_cast<float4 *>(n_vectors.p + t0 * stride);
				hipLaunchKernelGGL(k_compact_rows, dim3((uint32_t)std::min<uint64_t>((n + 3) / 4, 16384)), dim3(256), 0, stream, a,
				                   (uint32_t)t0, (uint32_t)n);
			}
			HIP_TRY(hipGetLastError());
		} else {
			// no second buffer (and therefore order kept): everything below the first tombstone stays; the rest moves DOWN
			// chunk by chunk through a staging buffer (a chunk's sources never lie below its destinations).  In place:
			// d_vectors is only rewritten here, after every other new array has been built; an error in this loop leaves rows
			// moved but the graph arrays untouched — vss_compact then reports the error and the index must be reloaded
			// (stated in vssgpu.h).
			const uint64_t chunk_rows = std::max<uint64_t>(1, std::min<uint64_t>((1ull << 30) / (stride * 4), live));
			HIP_TRY(hipStreamSynchronize(stream)); // links, keys and levels are complete before the first row moves
			if (first_moved < live) {
				staging.ensure(chunk_rows * stride, 0, stream);
				a.staging = reinterpret_cast<float4 *>(staging.p);
				for (uint64_t t0 = first_moved; t0 < live; t0 += chunk_rows) {
					const uint64_t n = std::min(chunk_rows, live - t0);
					const uint32_t gr = (uint32_t)std::min<uint64_t>((n + 3) / 4, 8192);
					hipLaunchKernelGGL(k_compact_rows, dim3(gr), dim3(256), 0, stream, a, (uint32_t)t0, (uint32_t)n);
					HIP_TRY(hipMemcpyAsync(d_vectors.p + t0 * stride, staging.p, n * stride * 4, hipMemcpyDeviceToDevice, stream));
				}
				HIP_TRY(hipGetLastError());
			}
			HIP_TRY(hipMemsetAsync(d_vectors.p + live * stride, 0, (count - live) * stride * 4, stream));
		}
		HIP_TRY(hipStreamSynchronize(stream));
	} catch (...) {
		drop_scratch();
		throw;
	}
	std::swap(d_links0, n_links0), std::swap(d_links_up, n_links_up), std::swap(d_list_owner, n_owner);
	std::swap(d_upper_off, n_upper_off), std::swap(d_levels, n_levels), std::swap(d_keys, n_keys);
	if (fresh_rows)
		std::swap(d_vectors, n_vectors);
	last_compact_reordered = reorder;
	drop_scratch();
	// host mirrors
	{
		std::vector<int64_t> nk(keys_h.size(), 0);
		std::vector<uint8_t> nl(levels_h.size(), 0);
		std::vector<uint32_t> no(upper_off_h.size(), 0);
		list_owner_h.assign(nup, 0);
		for (uint64_t t = 0; t != live; ++t) {
			const uint32_t sidx = src_of[t];
			nk[t] = keys_h[sidx];
			const uint8_t lv = levels_h[sidx];
			nl[t] = lv;
			no[t] = noff[t];
			for (int l = 0; l < lv; ++l)
				list_owner_h[noff[t] + l] = (uint32_t)t;
		}
		keys_h.swap(nk), levels_h.swap(nl), upper_off_h.swap(no);
	}
	count = live;
	n_upper = nup;
	tombstones = 0;
	free_slots.clear();
	max_level = live ? nml : -1;
	entry = nentry;
	keymap = KeyMap();
	mutations++;
	return VSS_OK;
}

// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------
#define VSS_GUARD_WITH(LOCK, index, ...)                                                                               \
	if (!(index))                                                                                                      \
		return VSS_ERROR;                                                                                              \
	LOCK _lk((index)->rw);                                                                                             \
	try {                                                                                                              \
		(void)hipSetDevice((index)->device);                                                                           \
		__VA_ARGS__                                                                                                    \
	} catch (const HipError &e) {                                                                                      \
		return (index)->fail("HIP error %d (%s) in %s", (int)e.code, hipGetErrorString(e.code), e.what);               \
	} catch (const std::exception &e) {                                                                                \
		return (index)->fail("%s", e.what());                                                                          \
	}
// calls that change the graph or its buffers: exclusive
#define VSS_GUARD(index, ...) VSS_GUARD_WITH(std::unique_lock<std::shared_mutex>, index, __VA_ARGS__)
// searches and read-only queries: any number at once
#define VSS_SHARED(index, ...) VSS_GUARD_WITH(std::shared_lock<std::shared_mutex>, index, __VA_ARGS__)

// ---- tuning options (vss_set_option; no reference counterpart: results never depend on any of them) --------------------------
// One entry per knob.  Round 6: rounds 2-5 exported a setter per knob — ten vss_set_search_* functions a
// DuckDB maintainer had to read past; they are this table now, and the environment variables of the same knobs (read once, in
// vss_create) go through the same checks: a value out of range is REFUSED and reported instead of being clamped silently.
namespace {
struct OptionRule {
	const char *name;
	int64_t lo, hi;
	void (*apply)(vss_index *, int64_t);
	const char *what;
};
const OptionRule OPTION_RULES[] = {
    {"search.waves", 2, 16, [](vss_index *h, int64_t v) { h->search_waves = (uint32_t)v; },
     "wavefronts per workgroup of the search engine"},
    {"search.walkers", 0, ENGINE_MAX_WALKERS, [](vss_index *h, int64_t v) { h->search_walkers = (uint32_t)v; },
     "walking waves among them (0 = chosen per launch); at least one scoring wave must remain"},
    {"search.solo", 0, 2, [](vss_index *h, int64_t v) { h->search_solo = (uint32_t)v; },
     "the one-wave-per-query shape: 0 never, 1 automatic, 2 always"},
    {"search.solo_max_queries", 1, 1 << 30, [](vss_index *h, int64_t v) { h->solo_max_queries = (uint32_t)v; },
     "largest launch the automatic rule gives the solo shape"},
    {"search.team", 0, 1, [](vss_index *h, int64_t v) { h->search_team = v != 0; }, "eight-wave teams in the solo shape"},
    {"search.crew", 0, 31,
     [](vss_index *h, int64_t v) {
	     h->search_crew = (v & 1) != 0;
	     if (v & 16) // explicit refinements (A/B measurements): bits 2-3 = CREW_SPARE_SIMD | CREW_NO_REQUESTS
		     h->search_crew_tune = (uint32_t)v & (CREW_SPARE_SIMD | CREW_NO_REQUESTS);
     },
     "the last walker of a workgroup runs its scoring waves as a crew (1 | 16 | refinement bits 4, 8)"},
    {"search.pipelined", 0, 1, [](vss_index *h, int64_t v) { h->search_pipelined = v != 0; }, "software-pipelined level search"},
    {"search.wide_lists", 0, 1, [](vss_index *h, int64_t v) { h->search_wide_lists = v != 0; },
     "limits of 257-512 in 12-wave workgroups with the pipelined level search"},
    {"search.visited_compact", 0, 1, [](vss_index *h, int64_t v) { h->visited_compact_on = v != 0; },
     "compact exact visited sets (16-bit cells) in LDS at limits of 257-512"},
    {"search.visited_lds_log2_max", 0, 14, [](vss_index *h, int64_t v) { h->hash_lds_max_override = (uint32_t)v; },
     "largest visited-set table (log2 of its 32-bit cells) kept in LDS with several walkers per workgroup; 0 = the engine's own "
     "(13); 1 = every such table in HBM"},
    {"search.visited_cells_per_limit", 0, 1 << 20, [](vss_index *h, int64_t v) { h->visited_per_limit = (uint64_t)v; },
     "visited-set cells per entry of the search limit; 0 = the sizing rule's own, else at least 4"},
    {"search.retry_in_place", 0, 1, [](vss_index *h, int64_t v) { h->retry_in_place = v != 0; },
     "a query that outgrows its LDS-resident visited set is repeated by its walker within the launch"},
    {"search.probe_flag_wait", 0, 1, [](vss_index *h, int64_t v) { h->probe_flag_wait = v != 0; },
     "host-pointer probes of at most 256 queries wait on a pinned flag instead of the stream"},
    {"search.lookahead", 0, ENGINE_MAX_WALKERS, [](vss_index *h, int64_t v) { h->search_spec_active = (uint32_t)v; },
     "one expansion of look-ahead while at most this many walkers of a workgroup still run (0 = off)"},
    {"search.gating", 0, 1, [](vss_index *h, int64_t v) { h->search_gating = v != 0; },
     "a launch is issued when its predecessor on the device starts to drain"},
    {"search.list_lds", 0, 2, [](vss_index *h, int64_t v) { h->search_list_lds = (uint32_t)v; },
     "candidate lists of limits 513-4096 in LDS: 0 never (HBM), 1 when the workgroup keeps its walkers, 2 whenever one walker fits"},
    {"search.prescore", 0, 2,
     [](vss_index *h, int64_t v) {
	     h->search_prescore = (uint32_t)v;
	     if (!h->search_prescore)
		     h->free_codes(); // 0: no codes are held, every job's bound is +inf — the path without the filter, exactly
	     else if (h->stream)
		     h->refresh_codes();
     },
     "scoring waves reject rows on exact bounds from 8-bit row codes before reading their f32 components: 0 never, 1 at limits of "
     "at most 256, 2 in every pipelined launch"},
    {"search.prescore_descent", 0, 1, [](vss_index *h, int64_t v) { h->search_prescore_descent = v != 0; },
     "in launches that filter on row codes, the greedy descent's rows are bounded against its closest distance too"},
};
// validated assignment (the caller holds the index exclusively, or is vss_create); nullptr = done, else why not
const char *set_option_checked(vss_index *h, const char *name, int64_t value) {
	for (const OptionRule &r : OPTION_RULES) {
		if (std::strcmp(r.name, name))
			continue;
		if (value < r.lo || value > r.hi)
			return "value out of range";
		if (!std::strcmp(name, "search.visited_cells_per_limit") && value != 0 && value < 4)
			return "value out of range";
		const uint32_t waves = !std::strcmp(name, "search.waves") ? (uint32_t)value : h->search_waves;
		const uint32_t walkers = !std::strcmp(name, "search.walkers") ? (uint32_t)value : h->search_walkers;
		if (walkers && walkers >= waves)
			return "at least one scoring wave must remain";
		r.apply(h, value);
		return nullptr;
	}
	return "no such option";
}
} // namespace

extern "C" {

const char *vss_version(void) {
	return "vssgpu 0.1 (gfx950, wave64)";
}

int vss_create(uint64_t dim, int metric, uint64_t M, uint64_t M0, uint64_t efc, uint64_t efs, int device,
               vss_index **out) {
	if (!out)
		return VSS_ERROR;
	*out = nullptr;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= device || device < 0) {
		fprintf(stderr, "vssgpu: no HIP device %d available (found %d) — the engine has no CPU fallback\n", device,
		        n_dev);
		return VSS_ERROR;
	}
	if (!dim || metric < 0 || metric > 2 || M < 2 || M0 < 2)
		return VSS_ERROR;
	if (M0 < M) {
		// usearch gives a new node up to M links on EVERY level, level 0 included (index.hpp:3665), and stores them in the
		// M0 cells of its base list: with M0 < M the reference itself writes past the list (heap corruption, observed with
		// the reference build).  There is nothing to be compatible with; refuse.
		fprintf(stderr, "vssgpu: M0 (%llu) must not be smaller than M (%llu)\n", (unsigned long long)M0,
		        (unsigned long long)M);
		return VSS_ERROR;
	}
	auto *h = new vss_index();
	h->device = device;
	h->configure(dim, metric, M, M0);
	h->efc = efc ? efc : 128;
	h->efs = efs ? efs : 64;
	if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
		delete h;
		return VSS_ERROR;
	}
	h->own_stream = true;
#ifdef VSS_PARANOID
	if (hipHostMalloc((void **)&h->h_debug, 128 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
		vss_destroy(h);
		return VSS_ERROR;
	}
	std::memset(h->h_debug, 0, 128 * sizeof(uint32_t));
#endif
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
		h->n_cus = (uint32_t)prop.multiProcessorCount;
	// A/B knobs from the environment (debugging and measurement sessions: tools/README.md).  Those that are options go through
	// vss_set_option's checks — a value out of range is refused and reported, never clamped silently.  Read ONCE,
	// here: setting them after vss_create has no effect on this index.
	static const struct { const char *env, *option; } ENV_OPTIONS[] = {
	    {"VSS_SEARCH_WAVES", "search.waves"}, {"VSS_SEARCH_WALKERS", "search.walkers"}, {"VSS_SEARCH_SPEC", "search.lookahead"},
	    {"VSS_SEARCH_SOLO", "search.solo"}, {"VSS_SEARCH_SOLO_MAX", "search.solo_max_queries"}, {"VSS_SEARCH_TEAM", "search.team"},
	    {"VSS_SEARCH_CREW", "search.crew"}, {"VSS_SEARCH_PIPELINED", "search.pipelined"},
	    {"VSS_SEARCH_WIDE_LISTS", "search.wide_lists"}, {"VSS_VISITED_COMPACT", "search.visited_compact"},
	    {"VSS_SEARCH_RETRY_IN_PLACE", "search.retry_in_place"}, {"VSS_HASH_LDS_MAX_LOG2", "search.visited_lds_log2_max"},
	    {"VSS_VISITED_PER_LIMIT", "search.visited_cells_per_limit"}, {"VSS_PROBE_FLAG_WAIT", "search.probe_flag_wait"},
	    {"VSS_SEARCH_LIST_LDS", "search.list_lds"}, {"VSS_SEARCH_PRESCORE", "search.prescore"},
	    {"VSS_SEARCH_PRESCORE_DESCENT", "search.prescore_descent"},
	};
	for (const auto &e : ENV_OPTIONS)
		if (const char *t = getenv(e.env)) {
			if (const char *why = set_option_checked(h, e.option, (int64_t)atoll(t)))
				fprintf(stderr, "vssgpu: %s=%s ignored (%s: %s)\n", e.env, t, e.option, why);
		}
	// debug-only knobs without an option (kernel selection, probes)
	if (const char *t = getenv("VSS_SEARCH_REG_QUEUE"))
		h->search_reg_queue = atoi(t) != 0;
	if (const char *t = getenv("VSS_SEARCH_REG_QUEUE_MAX"))
		h->reg_queue_max_limit = (uint32_t)std::max(0, std::min(64 * MAX_LIST_REGS, atoi(t)));
	if (const char *t = getenv("VSS_FORCE_LOOPING"))
		h->force_looping = atoi(t) != 0;
	if (const char *t = getenv("VSS_EXACT_PROBE"))
		h->exact_probe = (uint32_t)atoi(t);
	if (const char *t = getenv("VSS_EXACT_KERNEL"))
		h->exact_kernel = (uint32_t)std::max(1, std::min(5, atoi(t)));
	if (const char *t = getenv("VSS_SEARCH_WGS_PER_CU"))
		h->search_wgs_per_cu = (uint32_t)std::max(1, std::min(8, atoi(t)));
	if (const char *t = getenv("VSS_SEARCH_WALKERS_CAP"))
		h->search_walkers_cap = (uint32_t)std::max(1, std::min((int)ENGINE_MAX_WALKERS, atoi(t)));
	if (const char *t = getenv("VSS_EXACT_FILTER"))
		h->exact_filter = atoi(t) != 0;
	if (const char *t = getenv("VSS_EXACT_CERTIFY"))
		h->exact_certify = (uint32_t)std::max(1, std::min(2, atoi(t)));
	if (const char *t = getenv("VSS_EXACT_REDO_QT"))
		h->exact_redo_qt = (uint32_t)std::max(1, std::min(MS_QT, atoi(t)));
	if (const char *t = getenv("VSS_EXACT_FILTER_LIST_ENTRIES")) {
		const long long v = atoll(t);
		if (v < (long long)EXACT_FILTER_LIST_ENTRIES_MIN || v > (long long)EXACT_FILTER_LIST_ENTRIES_MAX)
			fprintf(stderr, "vssgpu: VSS_EXACT_FILTER_LIST_ENTRIES=%s ignored (%llu .. %llu list entries per pass)\n", t,
			        (unsigned long long)EXACT_FILTER_LIST_ENTRIES_MIN, (unsigned long long)EXACT_FILTER_LIST_ENTRIES_MAX);
		else
			h->exact_filter_budget = (uint64_t)v;
	}
	if (const char *t = getenv("VSS_SEARCH_CREW_TUNE"))
		h->search_crew_tune = (uint32_t)atoi(t) & (CREW_SPARE_SIMD | CREW_NO_REQUESTS);
	if (const char *t = getenv("VSS_SEARCH_TOUCH_LISTS"))
		h->search_touch_lists = atoi(t) != 0;
	if (const char *t = getenv("VSS_SEARCH_TOUCH_ROWS"))
		h->search_touch_rows = atoi(t) != 0;
	if (const char *t = getenv("VSS_SEARCH_TOUCH_MAX"))
		h->search_touch_max_queries = (uint32_t)std::max(0, atoi(t));
	*out = h;
	return VSS_OK;
}

void vss_destroy(vss_index *h) {
	if (!h)
		return;
	(void)hipSetDevice(h->device);
	{
		// nobody may be waiting on (or name) this index's contexts any more (an index launches on its own device only)
		DeviceGate &dg = g_gate[(unsigned)h->device % 64];
		std::lock_guard<std::mutex> lk(dg.mu);
		if (dg.last.owner == h)
			dg.last = GateEntry();
	}
	if (h->stream)
		(void)hipStreamSynchronize(h->stream);
	h->release();
	if (h->own_stream && h->stream)
		(void)hipStreamDestroy(h->stream);
	delete h;
}

const char *vss_last_error(vss_index *h) {
	return h ? tls_error.c_str() : "null index";
}

int vss_set_stream(vss_index *h, void *s) {
	VSS_GUARD(h, {
		HIP_TRY(hipStreamSynchronize(h->stream));
		if (s) {
			if (h->own_stream)
				(void)hipStreamDestroy(h->stream);
			h->stream = (hipStream_t)s;
			h->own_stream = false;
		} else if (!h->own_stream) {
			HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
			h->own_stream = true;
		}
		return VSS_OK;
	})
}

int vss_synchronize(vss_index *h) {
	VSS_GUARD(h, {
		HIP_TRY(hipStreamSynchronize(h->stream));
		return VSS_OK;
	})
}

int vss_reserve(vss_index *h, uint64_t members, uint64_t threads) {
	VSS_GUARD(h, {
		const int rc = h->reserve(members, threads);
		if (rc == VSS_OK && h->count)
			h->refresh_codes(); // (the rows moved to larger buffers: so do their codes)
		return rc;
	})
}

int vss_stage_batch(vss_index *h, const int64_t *rowids, const float *vecs, const uint64_t *validity, uint64_t n) {
	VSS_GUARD(h, { return h->stage(rowids, vecs, validity, n, false); })
}

int vss_stage_batch_device(vss_index *h, const int64_t *rowids, const float *vecs, uint64_t n) {
	VSS_GUARD(h, { return h->stage(rowids, vecs, nullptr, n, true); })
}

int vss_build_finalize(vss_index *h) {
	VSS_GUARD(h, {
		const int rc = h->build_finalize();
		if (rc == VSS_OK)
			h->refresh_codes();
		return rc;
	})
}

int vss_add_batch(vss_index *h, const int64_t *rowids, const float *vecs, const uint64_t *validity, uint64_t n) {
	VSS_GUARD(h, {
		int rc = h->stage(rowids, vecs, validity, n, false);
		if (rc != VSS_OK)
			return rc;
		rc = h->build_finalize();
		if (rc == VSS_OK)
			h->refresh_codes();
		return rc;
	})
}

int vss_set_build_reorder(vss_index *h, int on) {
	VSS_GUARD(h, {
		h->reorder_after_build = on != 0;
		return VSS_OK;
	})
}

int vss_set_build_params(vss_index *h, uint64_t max_batch, uint64_t growth_div) {
	VSS_GUARD(h, {
		if (!max_batch || !growth_div)
			return h->fail("max_batch and growth_div must be positive");
		h->max_batch = max_batch;
		h->growth_div = growth_div;
		return VSS_OK;
	})
}

#ifdef VSS_PARANOID
/* debug builds only: the 64 pinned words the kernels leave notes in (readable while a kernel runs) */
uint32_t *vss_debug_buffer(vss_index *h) {
	return h ? h->h_debug : nullptr;
}
#endif

int vss_set_option(vss_index *h, const char *name, int64_t value) {
	VSS_GUARD(h, {
		if (!name)
			return h->fail("vss_set_option: no option name");
		if (const char *why = set_option_checked(h, name, value))
			return h->fail("vss_set_option(\"%s\", %lld): %s", name, (long long)value, why);
		return VSS_OK;
	})
}

int vss_search(vss_index *h, const float *q, uint64_t k, uint64_t ef, int64_t *out, uint64_t *out_count) {
	VSS_SHARED(h, {
		uint32_t cnt = 0;
		int rc = h->search_host(q, 1, k, ef, out, nullptr, &cnt, false, SearchPredicate());
		if (out_count)
			*out_count = cnt;
		return rc;
	})
}

int vss_search_batch(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, int64_t *out, float *out_d,
                     uint32_t *out_counts) {
	VSS_SHARED(h, { return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false, SearchPredicate()); })
}

int vss_search_batch_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, int64_t *out,
                            float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, { return h->search_launch(h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts)); })
}

int vss_search_batch_filtered(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint64_t *allowed,
                              uint64_t n_bits, int64_t *out, float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, {
		if (!allowed)
			return h->fail("filtered search needs a row-id bitmap");
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false, SearchPredicate::one_bitmap(allowed, n_bits));
	})
}

int vss_search_batch_filtered_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                     const uint64_t *d_allowed, uint64_t n_bits, int64_t *out, float *out_d,
                                     uint32_t *out_counts) {
	VSS_SHARED(h, {
		if (!d_allowed)
			return h->fail("filtered search needs a row-id bitmap");
		SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
		r.predicate = SearchPredicate::one_bitmap(d_allowed, n_bits);
		return h->search_launch(r);
	})
}

// VSS_OK, or the rule of csrc/filter_groups.h that table `t` of `n_bits` bits per group breaks, in the engine's words: `what` is
// the entry point, `batch` the batch of a multi-batch launch the table belongs to, or -1 where the call has one table.
static int check_table(vss_index *h, const char *what, int64_t batch, const FilterGroupBatch &t, uint64_t n_bits,
                       bool group_of_required) {
	char who[40] = "filtered search";
	if (batch >= 0)
		std::snprintf(who, sizeof who, "batch %lld", (long long)batch);
	const FilterTableFault fault = check_filter_table(t.allowed, t.n_groups, n_bits, t.group_of, group_of_required);
	if (fault == FilterTableFault::NONE)
		return VSS_OK;
	if (fault == FilterTableFault::TOO_LARGE)
		return h->fail("%s: %s: %llu groups of %llu bits are more than a table can hold", what, who, (unsigned long long)t.n_groups,
		               (unsigned long long)n_bits);
	return h->fail("%s: %s needs %s", what, who,
	               fault == FilterTableFault::NO_GROUPS          ? "at least one group"
	               : fault == FilterTableFault::NO_GROUP_NUMBERS ? "the group of every query"
	               : batch < 0                                   ? "the groups' row-id bitmaps"
	                                                             : "its groups' row-id bitmaps");
}
// ... and the group numbers of a table, in HOST memory: refused before anything is uploaded or launched
static int check_group_numbers(vss_index *h, const char *what, const FilterGroupBatch &t, uint64_t nq) {
	const uint64_t bad = first_unknown_group(t.group_of, nq, t.n_groups);
	if (bad == NO_BAD_GROUP)
		return VSS_OK;
	return h->fail("%s: query %llu names group %u, the table holds %llu", what, (unsigned long long)bad, t.group_of[bad],
	               (unsigned long long)t.n_groups);
}

// Per-query predicates: ONE launch for a join chunk whose outer rows each carry their own WHERE (hnsw_optimize_join.cpp:111-168
// with a correlated predicate; the predicate itself is usearch's filtered_search, index_dense.hpp:625-629).
int vss_search_batch_filtered_groups(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                     const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of,
                                     int64_t *out, float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, {
		const char *what = "vss_search_batch_filtered_groups";
		const SearchPredicate filter = SearchPredicate::one_table(allowed, group_of, n_groups, n_bits);
		const FilterGroupBatch &table = filter.batches[0];
		if (nq && k && (check_table(h, what, -1, table, n_bits, true) != VSS_OK || check_group_numbers(h, what, table, nq) != VSS_OK))
			return VSS_ERROR;
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false, filter);
	})
}

int vss_search_batch_filtered_groups_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                            const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits,
                                            const uint32_t *group_of, int64_t *out, float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, {
		SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
		r.predicate = SearchPredicate::one_table(allowed, group_of, n_groups, n_bits);
		if (nq && k && check_table(h, "vss_search_batch_filtered_groups_device", -1, r.predicate.batches[0], n_bits, true) != VSS_OK)
			return VSS_ERROR;
		return h->search_launch(r);
	})
}

// the caller's contexts are 0 .. EXPLICIT_CTX-1; the others are leased internally by the host-pointer entry points
#define VSS_CHECK_CALLER_CONTEXT(h, context)                                                                           \
	if ((context) < 0 || (context) >= vss_index::EXPLICIT_CTX)                                                         \
		return (h)->fail("search context %d out of range (0..%d)", (int)(context), vss_index::EXPLICIT_CTX - 1);

int vss_search_batch_device_begin(vss_index *h, int context, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                  int64_t *out, float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, {
		VSS_CHECK_CALLER_CONTEXT(h, context)
		if (nq && k && (!Q || !out || !out_counts))
			return h->fail("vss_search_batch_device_begin: null query / row-id / count pointer");
		SearchRequest r = h->request(context, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
		r.gate = true;
		return h->search_begin(r);
	})
}

int vss_search_multi_device_begin(vss_index *h, int context, uint64_t n_batches, const float *const *Q, uint64_t per_batch,
                                  uint64_t k, uint64_t ef, int64_t *const *out, float *const *out_d,
                                  uint32_t *const *out_counts) {
	VSS_SHARED(h, {
		VSS_CHECK_CALLER_CONTEXT(h, context)
		if (!Q || !out || !out_d || !out_counts)
			return h->fail("vss_search_multi_device_begin: null table");
		if (n_batches < 1 || n_batches > MAX_COALESCED)
			return h->fail("1 to %d batches per launch", MAX_COALESCED);
		for (uint64_t b = 0; per_batch && k && b != n_batches; ++b) // only d_out_distances[b] may be NULL
			if (!Q[b] || !out[b] || !out_counts[b])
				return h->fail("vss_search_multi_device_begin: null query / row-id / count pointer for batch %llu",
				               (unsigned long long)b);
		SearchRequest r = h->request(context, Q, n_batches, per_batch, k, ef, out, out_d, out_counts);
		r.gate = true;
		return h->search_begin(r);
	})
}

// The filtered forms of the two calls above.  The caller's bitmaps, tables and group numbers are read by the launch AND by the
// re-run rounds of vss_search_batch_end: they stay the caller's, valid and unchanged, until that returns.
int vss_search_batch_filtered_device_begin(vss_index *h, int context, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                           const uint64_t *d_allowed, uint64_t n_bits, int64_t *out, float *out_d,
                                           uint32_t *out_counts) {
	VSS_SHARED(h, {
		VSS_CHECK_CALLER_CONTEXT(h, context)
		if (nq && k && (!Q || !out || !out_counts))
			return h->fail("vss_search_batch_filtered_device_begin: null query / row-id / count pointer");
		if (nq && k && !d_allowed)
			return h->fail("vss_search_batch_filtered_device_begin: filtered search needs a row-id bitmap");
		SearchRequest r = h->request(context, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
		r.gate = true;
		r.predicate = SearchPredicate::one_bitmap(d_allowed, n_bits);
		return h->search_begin(r);
	})
}

int vss_search_batch_filtered_groups_device_begin(vss_index *h, int context, const float *Q, uint64_t nq, uint64_t k,
                                                  uint64_t ef, const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits,
                                                  const uint32_t *group_of, int64_t *out, float *out_d,
                                                  uint32_t *out_counts) {
	VSS_SHARED(h, {
		VSS_CHECK_CALLER_CONTEXT(h, context)
		if (nq && k && (!Q || !out || !out_counts))
			return h->fail("vss_search_batch_filtered_groups_device_begin: null query / row-id / count pointer");
		SearchRequest r = h->request(context, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
		r.gate = true;
		r.predicate = SearchPredicate::one_table(allowed, group_of, n_groups, n_bits);
		if (nq && k && check_table(h, "vss_search_batch_filtered_groups_device_begin", -1, r.predicate.batches[0], n_bits, true) != VSS_OK)
			return VSS_ERROR;
		return h->search_begin(r);
	})
}

int vss_search_multi_filtered_device_begin(vss_index *h, int context, uint64_t n_batches, const float *const *Q,
                                           uint64_t per_batch, uint64_t k, uint64_t ef, const uint64_t *const *d_allowed,
                                           const uint64_t *n_groups, uint64_t n_bits, const uint32_t *const *d_group_of,
                                           int64_t *const *out, float *const *out_d, uint32_t *const *out_counts) {
	VSS_SHARED(h, {
		VSS_CHECK_CALLER_CONTEXT(h, context)
		if (!Q || !out || !out_d || !out_counts || !d_allowed || !n_groups || !d_group_of)
			return h->fail("vss_search_multi_filtered_device_begin: null table");
		if (n_batches < 1 || n_batches > MAX_COALESCED)
			return h->fail("1 to %d batches per launch", MAX_COALESCED);
		SearchRequest r = h->request(context, Q, n_batches, per_batch, k, ef, out, out_d, out_counts);
		r.gate = true;
		r.predicate.kind = SearchPredicate::PER_QUERY, r.predicate.n_bits = n_bits;
		bool one_bitmap = per_batch && k; // every batch filtered by the same single bitmap: a plain filtered launch
		for (uint64_t b = 0; per_batch && k && b != n_batches; ++b) {
			if (!Q[b] || !out[b] || !out_counts[b]) // only d_out_distances[b] may be NULL
				return h->fail("vss_search_multi_filtered_device_begin: null query / row-id / count pointer for batch %llu",
				               (unsigned long long)b);
			const FilterGroupBatch table = {d_allowed[b], d_group_of[b], n_groups[b]};
			if (check_table(h, "vss_search_multi_filtered_device_begin", (int64_t)b, table, n_bits, false) != VSS_OK)
				return VSS_ERROR;
			r.predicate.batches[b] = table;
			one_bitmap &= !d_group_of[b] && d_allowed[b] == d_allowed[0];
		}
		if (one_bitmap)
			r.predicate = SearchPredicate::one_bitmap(d_allowed[0], n_bits);
		return h->search_begin(r);
	})
}

int vss_search_batch_end(vss_index *h, int context) {
	VSS_SHARED(h, {
		VSS_CHECK_CALLER_CONTEXT(h, context)
		return h->search_end(context, false);
	})
}

int vss_search_exact_batch(vss_index *h, const float *Q, uint64_t nq, uint64_t k, int64_t *out, float *out_d,
                           uint32_t *out_counts) {
	VSS_SHARED(h, { return h->search_host(Q, nq, k, 0, out, out_d, out_counts, true, SearchPredicate()); })
}

int vss_search_exact_batch_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, int64_t *out, float *out_d,
                                  uint32_t *out_counts) {
	VSS_SHARED(h, { return h->exact_launch(Q, (uint32_t)h->dim, nq, k, out, out_d, out_counts); })
}

// Exact top-k under per-query predicates: only the rows a query's group admits are scored (exact_filtered_kernels.h).  The table
// and the admission rule are vss_search_batch_filtered_groups'; group_of == NULL gives every query bitmap 0.
static int check_exact_filtered(vss_index *h, const char *what, const float *Q, uint64_t nq, const FilterGroupBatch &table,
                                uint64_t n_bits, const int64_t *out, const uint32_t *out_counts) {
	if (!Q || !out || !out_counts)
		return h->fail("%s: null query / row-id / count pointer", what);
	if (check_table(h, what, -1, table, n_bits, false) != VSS_OK)
		return VSS_ERROR;
	if (nq > 0xFFFFFFFFull)
		return h->fail("%s: at most 2^32 - 1 queries per call", what);
	return VSS_OK;
}

int vss_search_exact_batch_filtered_groups(vss_index *h, const float *Q, uint64_t nq, uint64_t k, const uint64_t *allowed,
                                           uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of, int64_t *out,
                                           float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, {
		const char *what = "vss_search_exact_batch_filtered_groups";
		const FilterGroupBatch table = {allowed, group_of, n_groups};
		if (!nq || !k)
			return VSS_OK;
		if (check_exact_filtered(h, what, Q, nq, table, n_bits, out, out_counts) != VSS_OK ||
		    (group_of && check_group_numbers(h, what, table, nq) != VSS_OK))
			return VSS_ERROR;
		return h->exact_filtered_host({Q, nq, k, 0, out, out_d, out_counts, nullptr}, allowed, n_groups, n_bits, group_of);
	})
}

int vss_search_exact_batch_filtered_groups_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k,
                                                  const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits,
                                                  const uint32_t *group_of, int64_t *out, float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, {
		const FilterGroupBatch table = {allowed, group_of, n_groups};
		if (!nq || !k)
			return VSS_OK;
		if (check_exact_filtered(h, "vss_search_exact_batch_filtered_groups_device", Q, nq, table, n_bits, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		const std::vector<uint32_t> groups_h = h->words_to_host(group_of, nq); // (the plan reads the group numbers on the host)
		const HostWords groups(group_of ? groups_h.data() : nullptr);
		return h->exact_filtered_launch({0, Q, (uint32_t)h->dim, nq, k, 0},
		                                GroupedRows::bitmaps(allowed, n_groups, n_bits, groups, DeviceWords(group_of)), {out, out_d, out_counts});
	})
}

int vss_last_exact_filtered(vss_index *h, uint64_t *out4) {
	if (!h || !out4)
		return VSS_ERROR;
	std::lock_guard<std::mutex> lk(h->exact_mu);
	std::memcpy(out4, h->last_exact_filtered, sizeof h->last_exact_filtered);
	return VSS_OK;
}

// Per-query predicates, each group answered by the cheaper of the two calls above (filter_route.h has the rule).  route_c is an
// argument and not an option: no option changes an answer, and this value chooses between two answers.
int vss_search_batch_filtered_groups_auto(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                          const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of,
                                          uint64_t route_c, int64_t *out, float *out_d, uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		const char *what = "vss_search_batch_filtered_groups_auto";
		const FilterGroupBatch table = {allowed, group_of, n_groups};
		if (!nq || !k)
			return VSS_OK;
		if (check_exact_filtered(h, what, Q, nq, table, n_bits, out, out_counts) != VSS_OK ||
		    (group_of && check_group_numbers(h, what, table, nq) != VSS_OK))
			return VSS_ERROR;
		return h->filtered_auto_host({Q, nq, k, ef, out, out_d, out_counts, out_route}, allowed, n_groups, n_bits, group_of, route_c);
	})
}

int vss_search_batch_filtered_groups_auto_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                                 const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits,
                                                 const uint32_t *group_of, uint64_t route_c, int64_t *out, float *out_d,
                                                 uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		const FilterGroupBatch table = {allowed, group_of, n_groups};
		if (!nq || !k)
			return VSS_OK;
		if (check_exact_filtered(h, "vss_search_batch_filtered_groups_auto_device", Q, nq, table, n_bits, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		const std::vector<uint32_t> groups_h = h->words_to_host(group_of, nq); // (the rule and the plans read them on the host)
		const HostWords groups(group_of ? groups_h.data() : nullptr);
		std::vector<uint8_t> route;
		if (const int rc = h->filtered_auto({0, Q, (uint32_t)h->dim, nq, k, ef},
		                                    GroupedRows::bitmaps(allowed, n_groups, n_bits, groups, DeviceWords(group_of)), route_c,
		                                    {out, out_d, out_counts}, route))
			return rc;
		h->route_to_device(route, out_route);
		return VSS_OK;
	})
}

int vss_last_filter_route(vss_index *h, uint64_t *out8) {
	if (!h || !out8)
		return VSS_ERROR;
	std::lock_guard<std::mutex> lk(h->exact_mu);
	std::memcpy(out8, h->last_filter_route, sizeof h->last_filter_route);
	return VSS_OK;
}

// ---- the label column and the search by label (label_filter.h; include/vssgpu.h has the contract)
int vss_set_labels(vss_index *h, uint64_t first_rowid, const uint32_t *labels, uint64_t n) {
	VSS_GUARD(h, { return h->set_labels("vss_set_labels", 0, first_rowid, labels, n, false); })
}

int vss_set_labels_device(vss_index *h, uint64_t first_rowid, const uint32_t *d_labels, uint64_t n) {
	VSS_GUARD(h, { return h->set_labels("vss_set_labels_device", 0, first_rowid, d_labels, n, true); })
}

int vss_clear_labels(vss_index *h) {
	VSS_GUARD(h, {
		if (h->refuse_while_probing("vss_clear_labels") != VSS_OK)
			return VSS_ERROR;
		h->clear_labels();
		return VSS_OK;
	})
}

uint64_t vss_labelled_rows(const vss_index *h) {
	if (!h)
		return 0;
	std::shared_lock<std::shared_mutex> lk(const_cast<vss_index *>(h)->rw);
	return h->labelled_rows;
}

// ---- label columns 0 .. VSS_LABEL_COLUMNS_MAX - 1 (column 0 is the one above)
static_assert(LABEL_COLUMNS_MAX == VSS_LABEL_COLUMNS_MAX, "one cap, in the rule's header and in the C header");
int vss_set_label_column(vss_index *h, uint32_t column, uint64_t first_rowid, const uint32_t *labels, uint64_t n) {
	VSS_GUARD(h, { return h->set_labels("vss_set_label_column", column, first_rowid, labels, n, false); })
}

int vss_set_label_column_device(vss_index *h, uint32_t column, uint64_t first_rowid, const uint32_t *d_labels, uint64_t n) {
	VSS_GUARD(h, { return h->set_labels("vss_set_label_column_device", column, first_rowid, d_labels, n, true); })
}

int vss_clear_label_column(vss_index *h, uint32_t column) {
	VSS_GUARD(h, {
		if (column >= LABEL_COLUMNS_MAX)
			return h->fail("vss_clear_label_column: column %u is not below VSS_LABEL_COLUMNS_MAX (%u)", (unsigned)column,
			               (unsigned)LABEL_COLUMNS_MAX);
		if (h->refuse_while_probing("vss_clear_label_column") != VSS_OK)
			return VSS_ERROR;
		h->clear_label_column(column);
		return VSS_OK;
	})
}

int vss_set_label_column64(vss_index *h, uint32_t column, uint64_t first_rowid, const uint64_t *labels, uint64_t n) {
	VSS_GUARD(h, { return h->set_labels("vss_set_label_column64", column, first_rowid, labels, n, false, 2); })
}

int vss_set_label_column64_device(vss_index *h, uint32_t column, uint64_t first_rowid, const uint64_t *d_labels, uint64_t n) {
	VSS_GUARD(h, { return h->set_labels("vss_set_label_column64_device", column, first_rowid, d_labels, n, true, 2); })
}

uint32_t vss_label_column_width(const vss_index *h, uint32_t column) {
	if (!h || column >= LABEL_COLUMNS_MAX)
		return 0;
	std::shared_lock<std::shared_mutex> lk(const_cast<vss_index *>(h)->rw);
	return h->label_width[column];
}

uint64_t vss_label_column_rows(const vss_index *h, uint32_t column) {
	if (!h || column >= LABEL_COLUMNS_MAX)
		return 0;
	std::shared_lock<std::shared_mutex> lk(const_cast<vss_index *>(h)->rw);
	return const_cast<vss_index *>(h)->label_rows(column);
}

// what every form of the call refuses before it stages or launches anything
static int check_by_label(vss_index *h, const char *what, const float *Q, uint64_t nq, const uint32_t *want, int mode,
                          const int64_t *out, const uint32_t *out_counts) {
	if (mode != VSS_BY_LABEL_GRAPH && mode != VSS_BY_LABEL_EXACT && mode != VSS_BY_LABEL_AUTO)
		return h->fail("%s: mode %d is none of VSS_BY_LABEL_GRAPH (0), _EXACT (1), _AUTO (2)", what, mode);
	if (!h->d_labels.p)
		return h->fail("%s: the index has no label column (call vss_set_labels first; vss_load and vss_clear_labels drop it)", what);
	if (h->label_width[0] == 64)
		return h->fail("%s: label column 0 holds 64-bit cells, which this call cannot read (vss_search_batch_by_label_box64 can)", what);
	if (!Q || !want || !out || !out_counts)
		return h->fail("%s: null query / wanted-label / row-id / count pointer", what);
	if (nq > 0xFFFFFFFFull)
		return h->fail("%s: at most 2^32 - 1 queries per call", what);
	return VSS_OK;
}

int vss_search_batch_by_label(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *want, int mode,
                              uint64_t route_c, int64_t *out, float *out_d, uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		if (check_by_label(h, "vss_search_batch_by_label", Q, nq, want, mode, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		if (mode != VSS_BY_LABEL_GRAPH)
			return h->by_label_host({Q, nq, k, ef, out, out_d, out_counts, out_route}, mode == VSS_BY_LABEL_EXACT, want, route_c);
		if (out_route)
			std::memset(out_route, FILTER_ROUTE_GRAPH, nq);
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false, SearchPredicate::by_label(want, h->labelled_rows));
	})
}

int vss_search_batch_by_label_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *want,
                                     int mode, uint64_t route_c, int64_t *out, float *out_d, uint32_t *out_counts,
                                     uint8_t *out_route) {
	VSS_SHARED(h, {
		if (check_by_label(h, "vss_search_batch_by_label_device", Q, nq, want, mode, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		std::vector<uint8_t> route(nq, FILTER_ROUTE_GRAPH);
		if (mode == VSS_BY_LABEL_GRAPH) {
			SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
			r.predicate = SearchPredicate::by_label(want, h->labelled_rows);
			if (const int rc = h->search_launch(r))
				return rc;
		} else {
			const std::vector<uint32_t> want_h = h->words_to_host(want, nq); // (the plans read the wanted labels on the host)
			const DeviceWords d_want(mode == VSS_BY_LABEL_EXACT ? nullptr : want);
			if (const int rc = h->by_label_launch({0, Q, (uint32_t)h->dim, nq, k, ef}, HostWords(want_h.data()), d_want, route_c,
			                                      {out, out_d, out_counts}, route))
				return rc;
		}
		h->route_to_device(route, out_route);
		return VSS_OK;
	})
}

// ---- the search by label range: the mode is refused first, before anything is read or staged
static int check_by_label_range(vss_index *h, const char *what, const float *Q, uint64_t nq, const uint32_t *lo, const uint32_t *hi,
                                int mode, const int64_t *out, const uint32_t *out_counts) {
	if (mode != VSS_BY_LABEL_GRAPH && mode != VSS_BY_LABEL_EXACT && mode != VSS_BY_LABEL_AUTO)
		return h->fail("%s: mode %d is none of VSS_BY_LABEL_GRAPH (0), _EXACT (1), _AUTO (2)", what, mode);
	if (!h->d_labels.p)
		return h->fail("%s: the index has no label column (call vss_set_labels first; vss_load and vss_clear_labels drop it)", what);
	if (h->label_width[0] == 64)
		return h->fail("%s: label column 0 holds 64-bit cells, which this call cannot read (vss_search_batch_by_label_box64 can)", what);
	if (nq && (!lo || !hi))
		return h->fail("%s: null lo / hi pointer for %llu queries", what, (unsigned long long)nq);
	if (nq && (!Q || !out || !out_counts))
		return h->fail("%s: null query / row-id / count pointer", what);
	if (nq > 0xFFFFFFFFull)
		return h->fail("%s: at most 2^32 - 1 queries per call", what);
	return VSS_OK;
}

int vss_search_batch_by_label_range(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *lo,
                                    const uint32_t *hi, int mode, uint64_t route_c, int64_t *out, float *out_d, uint32_t *out_counts,
                                    uint8_t *out_route) {
	VSS_SHARED(h, {
		if (check_by_label_range(h, "vss_search_batch_by_label_range", Q, nq, lo, hi, mode, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		if (mode != VSS_BY_LABEL_GRAPH)
			return h->by_range_host({Q, nq, k, ef, out, out_d, out_counts, out_route}, mode == VSS_BY_LABEL_EXACT, lo, hi, route_c);
		if (out_route)
			std::memset(out_route, FILTER_ROUTE_GRAPH, nq);
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false, SearchPredicate::by_range(lo, hi, h->labelled_rows));
	})
}

int vss_search_batch_by_label_range_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *lo,
                                           const uint32_t *hi, int mode, uint64_t route_c, int64_t *out, float *out_d,
                                           uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		if (check_by_label_range(h, "vss_search_batch_by_label_range_device", Q, nq, lo, hi, mode, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		std::vector<uint8_t> route(nq, FILTER_ROUTE_GRAPH);
		if (mode == VSS_BY_LABEL_GRAPH) {
			SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
			r.predicate = SearchPredicate::by_range(lo, hi, h->labelled_rows);
			if (const int rc = h->search_launch(r))
				return rc;
		} else {
			// (the plans read the ends on the host)
			const std::vector<uint32_t> lo_h = h->words_to_host(lo, nq), hi_h = h->words_to_host(hi, nq);
			const bool exact = mode == VSS_BY_LABEL_EXACT;
			if (const int rc = h->by_range_launch({0, Q, (uint32_t)h->dim, nq, k, ef}, HostWords(lo_h.data()), HostWords(hi_h.data()),
			                                      DeviceWords(exact ? nullptr : lo), DeviceWords(exact ? nullptr : hi), route_c,
			                                      {out, out_d, out_counts}, route))
				return rc;
		}
		h->route_to_device(route, out_route);
		return VSS_OK;
	})
}

// ---- the search by label set: the mode is refused first, then the width, then null sets — all before anything is launched or
// written — and the missing column after them
static_assert(LABEL_SET_MAX == VSS_LABEL_SET_MAX, "one cap, in the rule's header and in the C header");
static int check_by_label_set(vss_index *h, const char *what, const float *Q, uint64_t nq, const uint32_t *sets, uint64_t width, int mode,
                              const int64_t *out, const uint32_t *out_counts) {
	if (mode != VSS_BY_LABEL_GRAPH && mode != VSS_BY_LABEL_EXACT && mode != VSS_BY_LABEL_AUTO)
		return h->fail("%s: mode %d is none of VSS_BY_LABEL_GRAPH (0), _EXACT (1), _AUTO (2)", what, mode);
	if (width < 1 || width > VSS_LABEL_SET_MAX)
		return h->fail("%s: width %llu is not within 1 .. VSS_LABEL_SET_MAX (%d); longer lists take the bitmap calls", what,
		               (unsigned long long)width, VSS_LABEL_SET_MAX);
	if (nq && !sets)
		return h->fail("%s: null sets pointer for %llu queries", what, (unsigned long long)nq);
	if (!h->d_labels.p)
		return h->fail("%s: the index has no label column (call vss_set_labels first; vss_load and vss_clear_labels drop it)", what);
	if (h->label_width[0] == 64)
		return h->fail("%s: label column 0 holds 64-bit cells, which this call cannot read (vss_search_batch_by_label_box64 can)", what);
	if (nq && (!Q || !out || !out_counts))
		return h->fail("%s: null query / row-id / count pointer", what);
	if (nq > 0xFFFFFFFFull)
		return h->fail("%s: at most 2^32 - 1 queries per call", what);
	return VSS_OK;
}

int vss_search_batch_by_label_set(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *sets, uint64_t width,
                                  int mode, uint64_t route_c, int64_t *out, float *out_d, uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		if (check_by_label_set(h, "vss_search_batch_by_label_set", Q, nq, sets, width, mode, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		if (mode != VSS_BY_LABEL_GRAPH)
			return h->by_set_host({Q, nq, k, ef, out, out_d, out_counts, out_route}, mode == VSS_BY_LABEL_EXACT, sets, (uint32_t)width,
			                      route_c);
		if (out_route)
			std::memset(out_route, FILTER_ROUTE_GRAPH, nq);
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false, SearchPredicate::by_set(sets, (uint32_t)width, h->labelled_rows));
	})
}

int vss_search_batch_by_label_set_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *sets,
                                         uint64_t width, int mode, uint64_t route_c, int64_t *out, float *out_d, uint32_t *out_counts,
                                         uint8_t *out_route) {
	VSS_SHARED(h, {
		if (check_by_label_set(h, "vss_search_batch_by_label_set_device", Q, nq, sets, width, mode, out, out_counts) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		std::vector<uint8_t> route(nq, FILTER_ROUTE_GRAPH);
		if (mode == VSS_BY_LABEL_GRAPH) {
			SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
			r.predicate = SearchPredicate::by_set(sets, (uint32_t)width, h->labelled_rows);
			if (const int rc = h->search_launch(r))
				return rc;
		} else {
			// (the plans read the sets on the host: nq x width words come back first)
			const std::vector<uint32_t> sets_h = h->words_to_host(sets, nq * width);
			const bool exact = mode == VSS_BY_LABEL_EXACT;
			if (const int rc = h->by_set_launch({0, Q, (uint32_t)h->dim, nq, k, ef}, HostWords(sets_h.data()), (uint32_t)width,
			                                    DeviceWords(exact ? nullptr : sets), route_c, {out, out_d, out_counts}, route))
				return rc;
		}
		h->route_to_device(route, out_route);
		return VSS_OK;
	})
}

// ---- the search by label box: the mode is refused first, then the number of columns, a null `columns`, a column out of range or
// named twice, null lo / hi — all before anything is launched or written — and a named column that was never set after them
// (wide_ok: the call reads 64-bit columns too — the box64 calls; the box calls refuse such a column right after an unset one)
static int check_by_label_box(vss_index *h, const char *what, const float *Q, uint64_t nq, const uint32_t *columns, uint64_t m,
                              const void *lo, const void *hi, int mode, const int64_t *out, const uint32_t *out_counts,
                              LabelBoxColumns &box, bool wide_ok = false) {
	if (mode != VSS_BY_LABEL_GRAPH && mode != VSS_BY_LABEL_EXACT && mode != VSS_BY_LABEL_AUTO)
		return h->fail("%s: mode %d is none of VSS_BY_LABEL_GRAPH (0), _EXACT (1), _AUTO (2)", what, mode);
	if (m < 1 || m > VSS_LABEL_COLUMNS_MAX)
		return h->fail("%s: n_columns %llu is not within 1 .. VSS_LABEL_COLUMNS_MAX (%d)", what, (unsigned long long)m,
		               VSS_LABEL_COLUMNS_MAX);
	if (!columns)
		return h->fail("%s: null columns pointer", what);
	if (const uint32_t bad = label_box_bad_column(columns, (uint32_t)m); bad != m)
		return columns[bad] >= LABEL_COLUMNS_MAX
		           ? h->fail("%s: column %u is not below VSS_LABEL_COLUMNS_MAX (%d)", what, (unsigned)columns[bad], VSS_LABEL_COLUMNS_MAX)
		           : h->fail("%s: column %u is named twice", what, (unsigned)columns[bad]);
	if (nq && (!lo || !hi))
		return h->fail("%s: null lo / hi pointer for %llu queries", what, (unsigned long long)nq);
	for (uint32_t j = 0; j != m; ++j)
		if (!h->label_cells(columns[j]).p)
			return h->fail("%s: the index has no label column %u (call vss_set_label_column first; vss_load, vss_clear_labels and "
			               "vss_clear_label_column drop it)", what, (unsigned)columns[j]);
	for (uint32_t j = 0; j != m && !wide_ok; ++j)
		if (h->label_width[columns[j]] == 64)
			return h->fail("%s: label column %u holds 64-bit cells, which this call cannot read (vss_search_batch_by_label_box64 can)", what,
			               (unsigned)columns[j]);
	if (nq && (!Q || !out || !out_counts))
		return h->fail("%s: null query / row-id / count pointer", what);
	if (nq > 0xFFFFFFFFull)
		return h->fail("%s: at most 2^32 - 1 queries per call", what);
	if (!h->named_label_columns(columns, m, box))
		return h->fail("%s: the named label columns cannot be read", what);
	return VSS_OK;
}

int vss_search_batch_by_label_box(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *columns,
                                  uint64_t n_columns, const uint32_t *lo, const uint32_t *hi, int mode, uint64_t route_c, int64_t *out,
                                  float *out_d, uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		LabelBoxColumns box;
		if (check_by_label_box(h, "vss_search_batch_by_label_box", Q, nq, columns, n_columns, lo, hi, mode, out, out_counts, box) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		std::vector<uint32_t> boxes;
		label_box_rows(lo, hi, nq, box.m, boxes);
		if (mode != VSS_BY_LABEL_GRAPH)
			return h->by_box_host({Q, nq, k, ef, out, out_d, out_counts, out_route}, mode == VSS_BY_LABEL_EXACT, boxes.data(), box, route_c);
		if (out_route)
			std::memset(out_route, FILTER_ROUTE_GRAPH, nq);
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false,
		                      SearchPredicate::by_box(boxes.data(), box.columns, box.m, box.shortest_rows()));
	})
}

int vss_search_batch_by_label_box_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *columns,
                                         uint64_t n_columns, const uint32_t *lo, const uint32_t *hi, int mode, uint64_t route_c,
                                         int64_t *out, float *out_d, uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		LabelBoxColumns box;
		if (check_by_label_box(h, "vss_search_batch_by_label_box_device", Q, nq, columns, n_columns, lo, hi, mode, out, out_counts, box) !=
		    VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		// the plans read the boxes on the host, and the walk reads them as ONE matrix of (lo, hi) pairs: both matrices come back
		// (8 * n_columns bytes per query) and go to context 0 interleaved
		const std::vector<uint32_t> lo_h = h->words_to_host(lo, nq * box.m), hi_h = h->words_to_host(hi, nq * box.m);
		std::vector<uint32_t> boxes;
		label_box_rows(lo_h.data(), hi_h.data(), nq, box.m, boxes);
		auto &c = h->context(0);
		const bool exact = mode == VSS_BY_LABEL_EXACT;
		if (!exact) {
			if (const int rc = h->stage_label_boxes(c, boxes.data(), box.m, nq))
				return rc;
			HIP_TRY(hipStreamSynchronize(c.stream)); // (`boxes` is pageable memory; the count kernels run on the index stream)
		}
		std::vector<uint8_t> route(nq, FILTER_ROUTE_GRAPH);
		if (mode == VSS_BY_LABEL_GRAPH) {
			SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
			r.predicate = SearchPredicate::by_box(c.d_group_of.p, box.columns, box.m, box.shortest_rows());
			if (const int rc = h->search_launch(r))
				return rc;
		} else if (const int rc = h->by_box_launch({0, Q, (uint32_t)h->dim, nq, k, ef}, HostWords(boxes.data()), box,
		                                           DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, {out, out_d, out_counts}, route))
			return rc;
		h->route_to_device(route, out_route);
		return VSS_OK;
	})
}

// ---- the search by label box64: the box call's checks in the box call's order (no width is refused), 64-bit ends
int vss_search_batch_by_label_box64(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *columns,
                                    uint64_t n_columns, const uint64_t *lo, const uint64_t *hi, int mode, uint64_t route_c, int64_t *out,
                                    float *out_d, uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		LabelBoxColumns box;
		if (check_by_label_box(h, "vss_search_batch_by_label_box64", Q, nq, columns, n_columns, lo, hi, mode, out, out_counts, box, true) !=
		    VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		std::vector<uint32_t> boxes;
		label_box64_rows(lo, hi, nq, box.m, boxes);
		if (mode != VSS_BY_LABEL_GRAPH)
			return h->by_box64_host({Q, nq, k, ef, out, out_d, out_counts, out_route}, mode == VSS_BY_LABEL_EXACT, boxes.data(), box, route_c);
		if (out_route)
			std::memset(out_route, FILTER_ROUTE_GRAPH, nq);
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false,
		                      SearchPredicate::by_box64(boxes.data(), box.columns, box.m, box.shortest_rows()));
	})
}

int vss_search_batch_by_label_box64_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, const uint32_t *columns,
                                           uint64_t n_columns, const uint64_t *lo, const uint64_t *hi, int mode, uint64_t route_c,
                                           int64_t *out, float *out_d, uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		LabelBoxColumns box;
		if (check_by_label_box(h, "vss_search_batch_by_label_box64_device", Q, nq, columns, n_columns, lo, hi, mode, out, out_counts, box,
		                       true) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		// the plans read the boxes on the host, and the walk reads them as ONE matrix of word pairs: both matrices come back
		// (16 * n_columns bytes per query) and go to context 0 as label_box64_rows lays them out
		const std::vector<uint32_t> lo_w = h->words_to_host(reinterpret_cast<const uint32_t *>(lo), 2 * nq * box.m),
		                            hi_w = h->words_to_host(reinterpret_cast<const uint32_t *>(hi), 2 * nq * box.m);
		std::vector<uint64_t> lo_h(nq * box.m), hi_h(nq * box.m);
		std::memcpy(lo_h.data(), lo_w.data(), lo_h.size() * 8), std::memcpy(hi_h.data(), hi_w.data(), hi_h.size() * 8);
		std::vector<uint32_t> boxes;
		label_box64_rows(lo_h.data(), hi_h.data(), nq, box.m, boxes);
		auto &c = h->context(0);
		const bool exact = mode == VSS_BY_LABEL_EXACT;
		if (!exact) {
			if (const int rc = h->stage_label_boxes(c, boxes.data(), box.m, nq, 2))
				return rc;
			HIP_TRY(hipStreamSynchronize(c.stream)); // (`boxes` is pageable memory; the count kernels run on the index stream)
		}
		std::vector<uint8_t> route(nq, FILTER_ROUTE_GRAPH);
		if (mode == VSS_BY_LABEL_GRAPH) {
			SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
			r.predicate = SearchPredicate::by_box64(c.d_group_of.p, box.columns, box.m, box.shortest_rows());
			if (const int rc = h->search_launch(r))
				return rc;
		} else if (const int rc = h->by_box64_launch({0, Q, (uint32_t)h->dim, nq, k, ef}, HostWords(boxes.data()), box,
		                                             DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, {out, out_d, out_counts}, route))
			return rc;
		h->route_to_device(route, out_route);
		return VSS_OK;
	})
}

// ---- the search by label set box: the mode is refused first, then the set width, the number of range columns, null sets / lo / hi,
// a column out of range, named twice or named beside the set column — all before anything is launched or written — then a column
// that was never set, then the null pointers and the query count every call by label refuses.  `box` names the set column first.
static int check_by_label_set_box(vss_index *h, const char *what, const float *Q, uint64_t nq, uint32_t set_column, const void *sets,
                                  uint32_t set_width, const uint32_t *columns, uint64_t m, const void *lo, const void *hi, int mode,
                                  const int64_t *out, const uint32_t *out_counts, LabelBoxColumns &box) {
	if (mode != VSS_BY_LABEL_GRAPH && mode != VSS_BY_LABEL_EXACT && mode != VSS_BY_LABEL_AUTO)
		return h->fail("%s: mode %d is none of VSS_BY_LABEL_GRAPH (0), _EXACT (1), _AUTO (2)", what, mode);
	if (set_width < 1 || set_width > VSS_LABEL_SET_MAX)
		return h->fail("%s: set_width %u is not within 1 .. VSS_LABEL_SET_MAX (%d); longer lists take the bitmap calls", what,
		               (unsigned)set_width, VSS_LABEL_SET_MAX);
	if (m > LABEL_SET_BOX_RANGES_MAX)
		return h->fail("%s: n_columns %llu is not within 0 .. %u (the set column takes one of the VSS_LABEL_COLUMNS_MAX slots)", what,
		               (unsigned long long)m, (unsigned)LABEL_SET_BOX_RANGES_MAX);
	if (nq && !sets)
		return h->fail("%s: null sets pointer for %llu queries", what, (unsigned long long)nq);
	if (nq && m && (!lo || !hi))
		return h->fail("%s: null lo / hi pointer for %llu queries", what, (unsigned long long)nq);
	if (m && !columns)
		return h->fail("%s: null columns pointer", what);
	if (const uint32_t bad = label_set_box_bad_column(set_column, columns, (uint32_t)m); bad != m + 1) {
		if (bad == 0)
			return h->fail("%s: set column %u is not below VSS_LABEL_COLUMNS_MAX (%d)", what, (unsigned)set_column, VSS_LABEL_COLUMNS_MAX);
		const uint32_t c = columns[bad - 1];
		return c >= LABEL_COLUMNS_MAX ? h->fail("%s: column %u is not below VSS_LABEL_COLUMNS_MAX (%d)", what, (unsigned)c, VSS_LABEL_COLUMNS_MAX)
		       : c == set_column      ? h->fail("%s: column %u is the set column and cannot carry a range too", what, (unsigned)c)
		                              : h->fail("%s: column %u is named twice", what, (unsigned)c);
	}
	uint32_t all[LABEL_COLUMNS_MAX] = {set_column};
	for (uint32_t j = 0; j != m; ++j)
		all[1 + j] = columns[j];
	for (uint32_t j = 0; j != m + 1; ++j)
		if (!h->label_cells(all[j]).p)
			return h->fail("%s: the index has no label column %u (call vss_set_label_column or vss_set_label_column64 first; vss_load, "
			               "vss_clear_labels and vss_clear_label_column drop it)", what, (unsigned)all[j]);
	if (nq && (!Q || !out || !out_counts))
		return h->fail("%s: null query / row-id / count pointer", what);
	if (nq > 0xFFFFFFFFull)
		return h->fail("%s: at most 2^32 - 1 queries per call", what);
	if (!h->named_label_columns(all, m + 1, box))
		return h->fail("%s: the named label columns cannot be read", what);
	return VSS_OK;
}

int vss_search_batch_by_label_set_box(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, uint32_t set_column,
                                      const uint64_t *sets, uint32_t set_width, const uint32_t *columns, uint64_t n_columns,
                                      const uint64_t *lo, const uint64_t *hi, int mode, uint64_t route_c, int64_t *out, float *out_d,
                                      uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		LabelBoxColumns box;
		if (check_by_label_set_box(h, "vss_search_batch_by_label_set_box", Q, nq, set_column, sets, set_width, columns, n_columns, lo, hi, mode,
		                           out, out_counts, box) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		std::vector<uint32_t> rows;
		label_set_box_rows(sets, set_width, lo, hi, nq, box.m - 1, rows);
		if (mode != VSS_BY_LABEL_GRAPH)
			return h->by_set_box_host({Q, nq, k, ef, out, out_d, out_counts, out_route}, mode == VSS_BY_LABEL_EXACT, rows.data(), set_width, box,
			                          route_c);
		if (out_route)
			std::memset(out_route, FILTER_ROUTE_GRAPH, nq);
		return h->search_host(Q, nq, k, ef, out, out_d, out_counts, false,
		                      SearchPredicate::by_set_box(rows.data(), set_width, box.columns, box.m, box.shortest_rows()));
	})
}

int vss_search_batch_by_label_set_box_device(vss_index *h, const float *Q, uint64_t nq, uint64_t k, uint64_t ef, uint32_t set_column,
                                             const uint64_t *sets, uint32_t set_width, const uint32_t *columns, uint64_t n_columns,
                                             const uint64_t *lo, const uint64_t *hi, int mode, uint64_t route_c, int64_t *out, float *out_d,
                                             uint32_t *out_counts, uint8_t *out_route) {
	VSS_SHARED(h, {
		LabelBoxColumns box;
		if (check_by_label_set_box(h, "vss_search_batch_by_label_set_box_device", Q, nq, set_column, sets, set_width, columns, n_columns, lo,
		                           hi, mode, out, out_counts, box) != VSS_OK)
			return VSS_ERROR;
		if (!nq || !k)
			return VSS_OK;
		// the plans read the predicates on the host, and the walk reads them as ONE matrix of travelling rows: the three matrices
		// come back (8 * (set_width + 2 * n_columns) bytes per query) and go to context 0 as label_set_box_rows lays them out
		const uint32_t m = box.m - 1;
		const auto to_host = [&](const uint64_t *d_words, uint64_t n) {
			const std::vector<uint32_t> w = h->words_to_host(reinterpret_cast<const uint32_t *>(d_words), 2 * n);
			std::vector<uint64_t> v(n);
			std::memcpy(v.data(), w.data(), n * 8);
			return v;
		};
		const std::vector<uint64_t> sets_h = to_host(sets, nq * set_width);
		const std::vector<uint64_t> lo_h = m ? to_host(lo, nq * m) : std::vector<uint64_t>(), hi_h = m ? to_host(hi, nq * m) : std::vector<uint64_t>();
		std::vector<uint32_t> rows;
		label_set_box_rows(sets_h.data(), set_width, lo_h.data(), hi_h.data(), nq, m, rows);
		auto &c = h->context(0);
		const bool exact = mode == VSS_BY_LABEL_EXACT;
		if (!exact) {
			if (const int rc = h->stage_label_set_boxes(c, rows.data(), label_set_box_row_words(set_width, m), nq))
				return rc;
			HIP_TRY(hipStreamSynchronize(c.stream)); // (`rows` is pageable memory; the count kernels run on the index stream)
		}
		std::vector<uint8_t> route(nq, FILTER_ROUTE_GRAPH);
		if (mode == VSS_BY_LABEL_GRAPH) {
			SearchRequest r = h->request(0, &Q, 1, nq, k, ef, &out, &out_d, &out_counts);
			r.predicate = SearchPredicate::by_set_box(c.d_group_of.p, set_width, box.columns, box.m, box.shortest_rows());
			if (const int rc = h->search_launch(r))
				return rc;
		} else if (const int rc = h->by_set_box_launch({0, Q, (uint32_t)h->dim, nq, k, ef}, HostWords(rows.data()), set_width, box,
		                                               DeviceWords(exact ? nullptr : c.d_group_of.p), route_c, {out, out_d, out_counts}, route))
			return rc;
		h->route_to_device(route, out_route);
		return VSS_OK;
	})
}

// ---- the six forms above in the pipelined and multi-batch launches: always the walk (mode graph), on the caller's context.
// Everything is refused HERE, before search_begin waits at the gate or enqueues anything: first what makes the batches of a launch
// differ (the message names the first batch that differs from batch 0), then, batch by batch, what the form's blocking call
// refuses, in its words, with the batch named after the entry point.
static_assert(VSS_LABEL_EQ == (int)LabelKind::EQ && VSS_LABEL_RANGE == (int)LabelKind::RANGE && VSS_LABEL_SET == (int)LabelKind::SET &&
                  VSS_LABEL_BOX == (int)LabelKind::BOX && VSS_LABEL_BOX64 == (int)LabelKind::BOX64 && VSS_LABEL_SET_BOX == (int)LabelKind::SET_BOX,
              "one numbering of the kinds, in the rule's header and in the C header");
static int label_begin(vss_index *h, const char *entry, bool multi, int context, uint64_t n_batches, const float *const *Q,
                       uint64_t per_batch, uint64_t k, uint64_t ef, const vss_label_predicate *preds, int64_t *const *out,
                       float *const *out_d, uint32_t *const *out_counts) {
	VSS_CHECK_CALLER_CONTEXT(h, context)
	if (!Q || !out || !out_d || !out_counts || !preds)
		return h->fail("%s: null table", entry);
	if (n_batches < 1 || n_batches > MAX_COALESCED)
		return h->fail("1 to %d batches per launch", MAX_COALESCED);
	const vss_label_predicate &p0 = preds[0];
	if (p0.kind < VSS_LABEL_EQ || p0.kind > VSS_LABEL_SET_BOX)
		return h->fail("%s: kind %d is none of VSS_LABEL_EQ (0) .. VSS_LABEL_SET_BOX (5)", entry, p0.kind);
	const bool has_set = p0.kind == VSS_LABEL_SET || p0.kind == VSS_LABEL_SET_BOX;
	const bool has_columns = p0.kind == VSS_LABEL_BOX || p0.kind == VSS_LABEL_BOX64 || p0.kind == VSS_LABEL_SET_BOX;
	for (uint64_t b = 1; b != n_batches; ++b) {
		const vss_label_predicate &p = preds[b];
		if (p.kind != p0.kind)
			return h->fail("%s: batch %llu is of kind %d, batch 0 of kind %d: one kind per launch", entry, (unsigned long long)b, p.kind, p0.kind);
		if (has_columns && (p.n_columns != p0.n_columns || (p0.kind == VSS_LABEL_SET_BOX && p.set_column != p0.set_column) ||
		                    !std::equal(p.columns, p.columns + std::min<uint32_t>(p.n_columns, VSS_LABEL_COLUMNS_MAX), p0.columns)))
			return h->fail("%s: batch %llu names other label columns than batch 0: the same columns, in the same order, per launch", entry,
			               (unsigned long long)b);
		if (has_set && p.set_width != p0.set_width)
			return h->fail("%s: batch %llu has set width %u, batch 0 has %u: one set width per launch", entry, (unsigned long long)b,
			               (unsigned)p.set_width, (unsigned)p0.set_width);
	}
	SearchRequest r = h->request(context, Q, n_batches, per_batch, k, ef, out, out_d, out_counts);
	r.gate = true;
	LabelBoxColumns box;
	SearchPredicate::LabelWords words[MAX_FILTER_GROUP_BATCHES] = {};
	// (as in the blocking calls, the checks do not depend on k, and with no queries only the pointers to them go unchecked)
	for (uint64_t b = 0; b != n_batches; ++b) {
		const vss_label_predicate &p = preds[b];
		char what[96];
		if (multi)
			std::snprintf(what, sizeof what, "%s: batch %llu", entry, (unsigned long long)b);
		else
			std::snprintf(what, sizeof what, "%s", entry);
		const int graph = VSS_BY_LABEL_GRAPH;
		int rc = VSS_OK;
		if (p.kind == VSS_LABEL_EQ)
			rc = check_by_label(h, what, Q[b], per_batch, static_cast<const uint32_t *>(p.d_want), graph, out[b], out_counts[b]);
		else if (p.kind == VSS_LABEL_RANGE)
			rc = check_by_label_range(h, what, Q[b], per_batch, static_cast<const uint32_t *>(p.d_lo), static_cast<const uint32_t *>(p.d_hi),
			                          graph, out[b], out_counts[b]);
		else if (p.kind == VSS_LABEL_SET)
			rc = check_by_label_set(h, what, Q[b], per_batch, static_cast<const uint32_t *>(p.d_sets), p.set_width, graph, out[b], out_counts[b]);
		else if (p.kind == VSS_LABEL_SET_BOX)
			rc = check_by_label_set_box(h, what, Q[b], per_batch, p.set_column, p.d_sets, p.set_width, p.columns, p.n_columns, p.d_lo, p.d_hi,
			                            graph, out[b], out_counts[b], box);
		else
			rc = check_by_label_box(h, what, Q[b], per_batch, p.columns, p.n_columns, p.d_lo, p.d_hi, graph, out[b], out_counts[b], box,
			                        p.kind == VSS_LABEL_BOX64);
		if (rc != VSS_OK)
			return rc;
		words[b] = {p.kind == VSS_LABEL_EQ ? p.d_want : p.d_sets, p.d_lo, p.d_hi};
	}
	if (per_batch && k) {
		if (p0.kind == VSS_LABEL_EQ)
			r.predicate = SearchPredicate::by_label(nullptr, h->labelled_rows).with_batches(words);
		else if (p0.kind == VSS_LABEL_RANGE)
			r.predicate = SearchPredicate::by_range(nullptr, nullptr, h->labelled_rows).with_batches(words);
		else if (p0.kind == VSS_LABEL_SET)
			r.predicate = SearchPredicate::by_set(nullptr, p0.set_width, h->labelled_rows).with_batches(words);
		else if (p0.kind == VSS_LABEL_BOX)
			r.predicate = SearchPredicate::by_box(nullptr, box.columns, box.m, box.shortest_rows()).with_batches(words);
		else if (p0.kind == VSS_LABEL_BOX64)
			r.predicate = SearchPredicate::by_box64(nullptr, box.columns, box.m, box.shortest_rows()).with_batches(words);
		else
			r.predicate = SearchPredicate::by_set_box(nullptr, p0.set_width, box.columns, box.m, box.shortest_rows()).with_batches(words);
	}
	return h->search_begin(r);
}

int vss_search_by_label_device_begin(vss_index *h, int context, const float *Q, uint64_t nq, uint64_t k, uint64_t ef,
                                     const vss_label_predicate *predicate, int64_t *out, float *out_d, uint32_t *out_counts) {
	VSS_SHARED(h, { return label_begin(h, "vss_search_by_label_device_begin", false, context, 1, &Q, nq, k, ef, predicate, &out, &out_d, &out_counts); })
}

int vss_search_multi_by_label_device_begin(vss_index *h, int context, uint64_t n_batches, const float *const *Q, uint64_t per_batch,
                                           uint64_t k, uint64_t ef, const vss_label_predicate *preds, int64_t *const *out,
                                           float *const *out_d, uint32_t *const *out_counts) {
	VSS_SHARED(h, {
		return label_begin(h, "vss_search_multi_by_label_device_begin", true, context, n_batches, Q, per_batch, k, ef, preds, out, out_d,
		                   out_counts);
	})
}

int vss_last_search_stats(vss_index *h, uint64_t *out4) {
	VSS_SHARED(h, {
		std::lock_guard<std::mutex> lk(h->stats_mu);
		std::memcpy(out4, h->last_stats, sizeof h->last_stats);
		return VSS_OK;
	})
}

int vss_last_search_prescore(vss_index *h, uint64_t *out4) {
	VSS_SHARED(h, {
		std::lock_guard<std::mutex> lk(h->stats_mu);
		std::memcpy(out4, h->last_prescore, sizeof h->last_prescore);
		return VSS_OK;
	})
}

int vss_last_search_prescore_descent(vss_index *h, uint64_t *out2) {
	VSS_SHARED(h, {
		std::lock_guard<std::mutex> lk(h->stats_mu);
		std::memcpy(out2, h->last_prescore_descent, sizeof h->last_prescore_descent);
		return VSS_OK;
	})
}

uint64_t vss_last_exact_fallbacks(vss_index *h) {
	if (!h)
		return 0;
	std::lock_guard<std::mutex> lk(h->exact_mu);
	return h->last_exact_fallbacks;
}

int vss_last_search_shape(vss_index *h, uint32_t *out8) {
	VSS_SHARED(h, {
		std::lock_guard<std::mutex> lk(h->stats_mu);
		std::memcpy(out8, h->last_shape, sizeof h->last_shape);
		return VSS_OK;
	})
}

/* debug builds only: per-query shader-clock ticks of the last search (VSS_PHASE_STRIDE values per query) */
#ifdef VSS_PHASE_TIMERS
int vss_debug_phase_ticks(vss_index *h, unsigned long long *out, uint64_t nq) {
	VSS_SHARED(h, {
		if (!h->ctx[0].d_phase.p || h->ctx[0].d_phase.n < nq * VSS_PHASE_STRIDE)
			return h->fail("no phase ticks recorded for %llu queries", (unsigned long long)nq);
		HIP_TRY(hipMemcpy(out, h->ctx[0].d_phase.p, nq * VSS_PHASE_STRIDE * 8, hipMemcpyDeviceToHost));
		return VSS_OK;
	})
}
#endif

int vss_build_work(vss_index *h, uint64_t *out3) {
	VSS_SHARED(h, {
		std::memset(out3, 0, 3 * sizeof(uint64_t));
		if (h->d_work_stats.p) {
			HIP_TRY(hipStreamSynchronize(h->stream));
			unsigned long long v[4];
			HIP_TRY(hipMemcpy(v, h->d_work_stats.p, sizeof v, hipMemcpyDeviceToHost));
			out3[0] = v[0];
			out3[1] = v[1];
			out3[2] = v[2];
		}
		return VSS_OK;
	})
}

int vss_timing(vss_index *h, double *out6, int reset) {
	VSS_SHARED(h, { // timing[] is guarded by stats_mu (searches) and written by the build only under the exclusive lock
		std::lock_guard<std::mutex> lk(h->stats_mu);
		std::memcpy(out6, h->timing, sizeof h->timing);
		if (reset)
			std::memset(h->timing, 0, sizeof h->timing);
		return VSS_OK;
	})
}

int vss_last_search_query_stats(vss_index *h, uint32_t *out, uint64_t nq) {
	VSS_SHARED(h, {
		std::lock_guard<std::mutex> lk(h->stats_mu);
		if (h->last_query_stats.size() < nq * 2)
			return h->fail("no per-query stats recorded for %llu queries", (unsigned long long)nq);
		std::memcpy(out, h->last_query_stats.data(), nq * 8);
		return VSS_OK;
	})
}

int vss_remove_batch(vss_index *h, const int64_t *rowids, uint64_t n, uint64_t *removed) {
	VSS_GUARD(h, { return h->remove(rowids, n, removed); })
}

int vss_compact(vss_index *h) {
	VSS_GUARD(h, {
		const int rc = h->compact(true);
		if (rc == VSS_OK)
			h->refresh_codes();
		return rc;
	})
}

int vss_compact_ex(vss_index *h, int reorder, int *out_reordered) {
	VSS_GUARD(h, {
		const int rc = h->compact(reorder != 0);
		if (rc == VSS_OK)
			h->refresh_codes();
		if (out_reordered)
			*out_reordered = rc == VSS_OK && h->last_compact_reordered ? 1 : 0;
		return rc;
	})
}

uint64_t vss_size(vss_index *h) {
	// live rows: linked and not tombstoned, plus every staged row — appended (`staged`) or taking over a tombstoned slot
	// (`n_pending`; `tombstones` still counts that slot until vss_build_finalize has re-linked it)
	return h ? h->count + h->staged + h->n_pending - h->tombstones : 0;
}
uint64_t vss_nodes(vss_index *h) {
	return h ? h->count + h->staged : 0;
}
uint64_t vss_capacity(vss_index *h) {
	return h ? h->capacity : 0;
}
int vss_build_progress(vss_index *h, uint64_t *linked, uint64_t *total) {
	if (!h)
		return VSS_ERROR;
	if (linked)
		*linked = h->progress_linked.load(std::memory_order_relaxed);
	if (total)
		*total = h->progress_total.load(std::memory_order_relaxed);
	return VSS_OK;
}
uint64_t vss_max_level(vss_index *h) {
	return (h && h->count) ? (uint64_t)h->max_level : 0;
}
uint64_t vss_dimensions(vss_index *h) {
	return h ? h->dim : 0;
}
int vss_metric(vss_index *h) {
	return h ? h->metric : -1;
}
uint64_t vss_memory_usage(vss_index *h) {
	if (!h)
		return 0;
	// what the contexts keep for vss_search_batch_filtered_groups (they grow and are reused): searches on other threads grow
	// them, so the sum is kept in an atomic and not read off the buffers
	const uint64_t group_tables = h->group_table_bytes.load(std::memory_order_relaxed);
	return h->d_vectors.n * 4 + h->d_links0.n * 4 + h->d_links_up.n * 4 + h->d_upper_off.n * 4 + h->d_levels.n +
	       h->d_keys.n * 8 + h->d_list_owner.n * 4 + h->d_codes.n * sizeof(uint32_t) + h->d_code_meta.n * sizeof(RowCodeMeta) +
	       group_tables + h->exact_filter_bytes.load(std::memory_order_relaxed) + h->label_bytes.load(std::memory_order_relaxed);
}

int vss_level_stats(vss_index *h, uint64_t level, uint64_t *out4) {
	VSS_SHARED(h, {
		HIP_TRY(hipStreamSynchronize(h->stream));
		h->level_stats(level, out4);
		return VSS_OK;
	})
}

uint64_t vss_serialized_length(vss_index *h) {
	return h ? h->serialized_length() : 0;
}

int vss_save(vss_index *h, vss_write_cb write, void *ctx) {
	// read-only: a checkpoint does not stall concurrent searches (two saves at once are fine too: each syncs the stream
	// for its own copies)
	VSS_SHARED(h, { return h->save(write, ctx); })
}

int vss_load(vss_index *h, vss_read_cb read, void *ctx) {
	VSS_GUARD(h, {
		const int rc = h->load(read, ctx);
		if (rc == VSS_OK) {
			h->clear_labels(); // (the stream's row ids are another table's: the caller sets its labels again)
			h->refresh_codes();
		}
		return rc;
	})
}

static int distance_launch(int fn, const float *a, const float *b, int b_const, uint64_t rows, uint64_t dim,
                           float *out, hipStream_t s) {
	if (fn < 0 || fn > 2 || !dim)
		return VSS_ERROR;
	if (!rows)
		return VSS_OK;
	const bool vec4 = (dim % 4 == 0) && ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0);
	const uint64_t units = vec4 ? dim / 4 : dim;
	const uint32_t G = (uint32_t)std::min<size_t>(64, ceil_pow2(units));
	const uint32_t logG = log2u(G);
	const uint64_t rows_per_block = 4 * (64 / G);
	const uint32_t grid = (uint32_t)std::min<uint64_t>((rows + rows_per_block - 1) / rows_per_block, 8192);
	if (vec4)
		hipLaunchKernelGGL(k_array_distance<true>, dim3(grid), dim3(256), 0, s, fn, a, b, b_const, rows, (uint32_t)dim,
		                   G, logG, out);
	else
		hipLaunchKernelGGL(k_array_distance<false>, dim3(grid), dim3(256), 0, s, fn, a, b, b_const, rows,
		                   (uint32_t)dim, G, logG, out);
	return hipGetLastError() == hipSuccess ? VSS_OK : VSS_ERROR;
}

int vss_distance_batch_device(int fn, const float *a, const float *b, int b_const, uint64_t rows, uint64_t dim,
                              float *out, void *stream) {
	return distance_launch(fn, a, b, b_const, rows, dim, out, (hipStream_t)stream);
}

// Host-pointer form: what a DuckDB scalar function sees is one <= 2048-row chunk of pageable host memory per call (SURVEY §8
// a13).  Round 6: the device buffers and the stream of a calling thread are kept between calls (grow-only, per thread and
// device) — rounds 1-5 paid three hipMalloc / hipFree pairs per chunk, which cost more than the chunk's transfer — and the
// operands travel as two asynchronous copies on that stream, the result as one.
namespace {
struct DistanceScratch {
	int device = -1;
	hipStream_t stream = nullptr;
	float *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
	uint64_t cap_a = 0, cap_b = 0, cap_out = 0; // floats
	void release() {
		if (device >= 0 && hipSetDevice(device) == hipSuccess) {
			(void)hipFree(d_a), (void)hipFree(d_b), (void)hipFree(d_out);
			if (stream)
				(void)hipStreamDestroy(stream);
		}
		d_a = d_b = d_out = nullptr, stream = nullptr, cap_a = cap_b = cap_out = 0, device = -1;
	}
	static bool grow(float *&p, uint64_t &cap, uint64_t want) {
		if (want <= cap)
			return true;
		(void)hipFree(p);
		p = nullptr, cap = 0;
		const uint64_t n = std::max<uint64_t>(want, 1u << 16);
		if (hipMalloc(&p, n * 4 + 16) != hipSuccess)
			return false;
		cap = n;
		return true;
	}
	~DistanceScratch() {
		release(); // (a thread that ends after the HIP runtime has been torn down gets errors back, nothing else)
	}
};
thread_local DistanceScratch t_distance;
} // namespace

int vss_distance_batch(int fn, const float *a, const float *b, int b_const, uint64_t rows, uint64_t dim, float *out,
                       int device) {
	if (hipSetDevice(device) != hipSuccess) {
		fprintf(stderr, "vssgpu: no HIP device %d — the engine has no CPU fallback\n", device);
		return VSS_ERROR;
	}
	if (fn < 0 || fn > 2 || !dim)
		return VSS_ERROR;
	if (!rows)
		return VSS_OK;
	DistanceScratch &sc = t_distance;
	if (sc.device != device) {
		sc.release();
		if (hipStreamCreateWithFlags(&sc.stream, hipStreamNonBlocking) != hipSuccess)
			return VSS_ERROR;
		sc.device = device;
	}
	const uint64_t nb = b_const ? dim : rows * dim;
	if (!DistanceScratch::grow(sc.d_a, sc.cap_a, rows * dim) || !DistanceScratch::grow(sc.d_b, sc.cap_b, nb) ||
	    !DistanceScratch::grow(sc.d_out, sc.cap_out, rows))
		return VSS_ERROR;
	int rc = VSS_ERROR;
	if (hipMemcpyAsync(sc.d_a, a, rows * dim * 4, hipMemcpyHostToDevice, sc.stream) == hipSuccess &&
	    hipMemcpyAsync(sc.d_b, b, nb * 4, hipMemcpyHostToDevice, sc.stream) == hipSuccess) {
		rc = distance_launch(fn, sc.d_a, sc.d_b, b_const, rows, dim, sc.d_out, sc.stream);
		if (rc == VSS_OK && hipMemcpyAsync(out, sc.d_out, rows * 4, hipMemcpyDeviceToHost, sc.stream) != hipSuccess)
			rc = VSS_ERROR;
	}
	if (hipStreamSynchronize(sc.stream) != hipSuccess)
		rc = VSS_ERROR;
	return rc;
}

// one 64-thread workgroup per query; the query's cells staged in LDS when they fit (exact_kernels.h: k_merge_topk)
static int merge_launch(const float *d, const int64_t *ids, size_t stride_d, size_t stride_id, uint64_t n_shards, uint64_t nq,
                        uint64_t k, float *out_d, int64_t *out_id, uint32_t *out_count, void *stream) {
	if (n_shards == 0 || n_shards * k > 0xFFFFFFFFull || nq > 0x7FFFFFFFull)
		return VSS_ERROR;
	const uint32_t head = ((uint32_t)n_shards * 4u + 15u) & ~15u;
	const uint64_t staged = head + n_shards * k * 12;
	if (staged <= vss::MERGE_STAGE_MAX_BYTES)
		hipLaunchKernelGGL(k_merge_topk<true>, dim3((uint32_t)nq), dim3(64), (uint32_t)staged, (hipStream_t)stream, d, ids, stride_d,
		                   stride_id, (uint32_t)n_shards, (uint32_t)nq, (uint32_t)k, out_d, out_id, out_count);
	else
		hipLaunchKernelGGL(k_merge_topk<false>, dim3((uint32_t)nq), dim3(64), head, (hipStream_t)stream, d, ids, stride_d, stride_id,
		                   (uint32_t)n_shards, (uint32_t)nq, (uint32_t)k, out_d, out_id, out_count);
	return hipGetLastError() == hipSuccess ? VSS_OK : VSS_ERROR;
}

int vss_merge_topk_device(const float *in_d, const int64_t *in_id, uint64_t n_shards, uint64_t nq, uint64_t k,
                          float *out_d, int64_t *out_id, uint32_t *out_count, void *stream) {
	if (!nq || !k)
		return VSS_OK;
	return merge_launch(in_d, in_id, (size_t)(nq * k), (size_t)(nq * k), n_shards, nq, k, out_d, out_id, out_count, stream);
}

uint64_t vss_packed_block_bytes(uint64_t nq, uint64_t k) {
	return (nq * k * 12 + 15) & ~15ull;
}

int vss_merge_topk_packed_device(const void *packed, uint64_t n_shards, uint64_t nq, uint64_t k, float *out_d,
                                 int64_t *out_id, uint32_t *out_count, void *stream) {
	if (!nq || !k)
		return VSS_OK;
	if ((uintptr_t)packed % 16)
		return VSS_ERROR;
	const uint64_t block = vss_packed_block_bytes(nq, k);
	const int64_t *ids = reinterpret_cast<const int64_t *>(packed);
	const float *d = reinterpret_cast<const float *>(reinterpret_cast<const unsigned char *>(packed) + nq * k * 8);
	return merge_launch(d, ids, (size_t)(block / 4), (size_t)(block / 8), n_shards, nq, k, out_d, out_id, out_count, stream);
}
}
