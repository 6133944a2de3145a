// host_logic.h — the pure host-side logic of the engine: no HIP, no device state, so that it can be compiled and tested
// on a CPU (tests/host_logic_probe.cpp, tests/test_host_logic.py) against the oracle and the reference build.
//
//   LevelRng        the reference's level generator (libstdc++ minstd_rand0 + generate_canonical<double,53>)
//   FreeRing        usearch's ring_gt as index_dense uses it for freed slots, wrap quirk included
//   KeyMap          rowid -> slot (lazy; deletes and duplicate checks)
//   batch_schedule  how a bulk build is cut into batch-synchronous steps
//   plan_search_launch  THE one place where a launch of the search engine is decided (shape, visited set, candidate list,
//                   scoring options, HBM scratch), over the rules before it (visited_set_log2, compact_visited_cells_log2,
//                   candidate_list_placement, the search shape) and the kernels' own LDS formulas (engine_layout.h)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "engine_layout.h"
#include "lds_list_index.h"
#include "visited_compact.h"

namespace vss {
namespace host {

constexpr int64_t FREE_KEY_HOST = 0x7FFFFFFFFFFFFFFFll; // = VSS_FREE_KEY (include/vssgpu.h), usearch's free_key_
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;               // = vss::EMPTY_SLOT

inline size_t ceil_pow2(size_t v) {
	size_t p = 1;
	while (p < v)
		p <<= 1;
	return p;
}
inline uint32_t log2u(size_t v) {
	uint32_t l = 0;
	while ((size_t(1) << l) < v)
		l++;
	return l;
}

// Level generator: libstdc++'s std::default_random_engine + uniform_real_distribution<double>, as used by
// usearch choose_random_level_ (index.hpp:3723-3727).  One stream per index (the reference keeps one per thread
// context, all identically seeded — SURVEY A.2); restarted by every growing reserve.
struct LevelRng {
	uint64_t x = 1;
	uint32_t next() {
		x = (x * 16807ull) % 2147483647ull;
		return (uint32_t)x;
	}
	double canonical() {
		const long double R = 2147483646.0L;
		double sum = 0, tmp = 1;
		for (int k = 0; k != 2; ++k) {
			sum += double(next() - 1u) * tmp;
			tmp = (double)((long double)tmp * R);
		}
		double ret = sum / tmp;
		if (ret >= 1.0)
			ret = std::nextafter(1.0, 0.0);
		return ret;
	}
	int level(double inv_log_m) {
		double r = -std::log(canonical()) * inv_log_m;
		return (int)(int16_t)r;
	}
	// the level as the engine stores it (u8)
	uint8_t stored_level(double inv_log_m) {
		const int lv = level(inv_log_m);
		return (uint8_t)(lv < 0 ? 0 : lv > 255 ? 255 : lv);
	}
};
inline double inverse_log_connectivity(uint64_t M) { // usearch index.hpp:3549
	return 1.0 / std::log((double)M);
}

// rowid -> slot, open addressing; built lazily (only deletes and duplicate checks need it)
struct KeyMap {
	std::vector<int64_t> k;
	std::vector<uint32_t> v;
	size_t mask = 0, used = 0;
	bool ready = false;
	static uint64_t hash(int64_t key) {
		uint64_t z = (uint64_t)key + 0x9E3779B97F4A7C15ull;
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		return z ^ (z >> 31);
	}
	void init(size_t n) {
		size_t cap = ceil_pow2(std::max<size_t>(16, n * 2));
		k.assign(cap, FREE_KEY_HOST);
		v.assign(cap, 0);
		mask = cap - 1;
		used = 0;
		ready = true;
	}
	void grow() {
		std::vector<int64_t> ok;
		std::vector<uint32_t> ov;
		ok.swap(k);
		ov.swap(v);
		init(ok.size());
		for (size_t i = 0; i != ok.size(); ++i)
			if (ok[i] != FREE_KEY_HOST && ov[i] != NO_SLOT)
				put(ok[i], ov[i]);
	}
	void put(int64_t key, uint32_t slot) {
		if ((used + 1) * 2 > k.size())
			grow();
		size_t h = hash(key) & mask;
		while (k[h] != FREE_KEY_HOST && k[h] != key)
			h = (h + 1) & mask;
		if (k[h] == FREE_KEY_HOST)
			used++;
		k[h] = key;
		v[h] = slot;
	}
	bool find(int64_t key, uint32_t &slot) const {
		size_t h = hash(key) & mask;
		while (k[h] != FREE_KEY_HOST) {
			if (k[h] == key) {
				slot = v[h];
				return slot != NO_SLOT;
			}
			h = (h + 1) & mask;
		}
		return false;
	}
	void erase(int64_t key) { // keep the key as a probe-chain marker, drop the slot
		size_t h = hash(key) & mask;
		while (k[h] != FREE_KEY_HOST) {
			if (k[h] == key) {
				v[h] = NO_SLOT;
				return;
			}
			h = (h + 1) & mask;
		}
	}
};

// The free list of tombstoned slots.  Restates usearch's ring_gt (index.hpp:1150-1277) as index_dense uses it
// (free_keys_, index_dense.hpp:463) INCLUDING its size() == 0 when the ring is exactly full: the order in which removed
// slots are handed back to later inserts is part of the reference's observable behaviour (which slot a row lands in).
struct FreeRing {
	std::vector<uint32_t> el;
	size_t cap = 0, head = 0, tail = 0;
	bool empty = true;
	size_t size() const {
		if (empty)
			return 0;
		return head >= tail ? head - tail : cap - (tail - head);
	}
	bool try_pop(uint32_t &v) {
		if (empty)
			return false;
		v = el[tail];
		tail = (tail + 1) % cap;
		empty = head == tail;
		return true;
	}
	void push(uint32_t v) {
		el[head] = v;
		head = (head + 1) % cap;
		empty = false;
	}
	bool reserve(size_t n) {
		if (n < size())
			return false;
		if (n <= cap)
			return true;
		n = std::max<size_t>(ceil_pow2(n), 64);
		std::vector<uint32_t> grown(n);
		size_t i = 0;
		while (try_pop(grown[i]))
			i++;
		el.swap(grown);
		cap = n, head = i, tail = 0;
		empty = i == 0;
		return true;
	}
	void clear() {
		head = tail = 0;
		empty = true;
	}
};


// Batch schedule of the bulk build (mirrored by oracle/hnsw_oracle.cpp `schedule`): batch = clamp(nodes / growth_div, 1,
// max_batch); a row whose level exceeds the current top level runs alone and becomes the entry (index.hpp:2769-2772).
// solo_row: the row that re-links the current entry slot, if any.  Its lists are blank while it is being re-linked, so
// batch mates descending from the entry would find nothing but the entry: it runs alone, like a level promotion.
inline std::vector<uint64_t> batch_schedule(uint64_t existing, int cur_max_level, const uint8_t *lv, uint64_t n,
                                      uint64_t max_batch, uint64_t growth_div, uint64_t solo_row = ~0ull) {
	std::vector<uint64_t> sizes;
	uint64_t i = 0, cur = existing;
	int ml = cur_max_level;
	while (i < n) {
		uint64_t b = 1;
		if (cur != 0) {
			b = std::max<uint64_t>(1, std::min(max_batch, cur / growth_div));
			uint64_t take = 0;
			while (take < b && i + take < n) {
				if ((int)lv[i + take] > ml || i + take == solo_row) {
					if (take == 0)
						take = 1;
					break;
				}
				take++;
			}
			b = take;
		}
		for (uint64_t j = 0; j != b; ++j)
			ml = std::max<int>(ml, lv[i + j]);
		sizes.push_back(b);
		i += b;
		cur += b;
	}
	return sizes;
}

// ---------------------------------------------------------------------------------------------------------
// Capacity of a walker's visited set (log2 of its cells; no reference counterpart — usearch's growing_hash_set_gt grows on
// demand, index.hpp:1018-1144; here a query that fills its table beyond 7/8 is re-run with a larger one).
//   per_limit  cells per entry of the search / insert limit: 64 is a table no ordinary query fills (the build, searches up to
//              limit 128 and beyond 256); searches with limits 129-256 take 32 — half the table, which stays in LDS (2^13
//              cells = 32 KiB, four walkers per workgroup) where 64 would push it to HBM and make every probe round an L2 /
//              memory round trip (the 2-74 queries of 10 240 that outgrow it are re-run)
//   bump       added after an overflow (the retry also carries a floor: strictly larger than the table that overflowed)
//   max_log2   "every node fits below 7/8": a table of that size cannot overflow
// ---------------------------------------------------------------------------------------------------------
inline uint64_t search_cells_per_limit(uint64_t limit) {
	return (limit > 128 && limit <= 256) ? 32 : 64;
}
inline uint32_t visited_set_log2(uint64_t limit, uint32_t bump, uint64_t M0, uint64_t list_cap_max, uint64_t per_limit,
                                 uint32_t max_log2) {
	uint64_t cap = ceil_pow2(per_limit * std::max<uint64_t>(std::min<uint64_t>(limit, 1u << 20), 2 * M0));
	cap = std::max<uint64_t>(cap, ceil_pow2(8ull * list_cap_max));
	cap = std::max<uint64_t>(cap, 1024);
	return std::min<uint32_t>(log2u(cap) + bump, max_log2);
}

// The compact visited set (visited_compact.h; 16-bit cells: tag + displacement, exact): taken by a launch of the workgroup
// engine whose 32-bit table would not fit LDS, when the limit is one of the 8-register list's (257-512: the only instantiation
// that carries the code), every slot fits 25 bits (24 until round 6) and this is the query's FIRST pass at the host's hands (a
// query whose set outgrows the cells — too many visits, a displacement beyond its bits — moves it to a plain table in HBM on the
// device, VisitedSet::migrate; one that outgrows that too is re-run by the host with the plain 32-bit table like any other
// overflow).  Returns the set's FORM (visited_compact.h: log2 of its cells — twice the words of the 32-bit table of
// 2^lds_table_log2 words it lies over — in bits 0-7, the key bits in bits 8-15 when they are not 24), or 0 = the plain set.
inline uint32_t compact_visited_cells_log2(bool plain_table_fits_lds, bool solo_shape, bool register_list, uint64_t limit,
                                           uint64_t nodes, bool first_pass, uint32_t lds_table_log2) {
	if (plain_table_fits_lds || solo_shape || !register_list || limit <= 256 || !first_pass)
		return 0;
	if (nodes > (1ull << compact_visited::KEY_BITS_MAX))
		return 0;
	const uint32_t cells_log2 = lds_table_log2 + 1;
	const uint32_t form = nodes > (1ull << compact_visited::KEY_BITS) ? compact_visited::make_form(cells_log2, compact_visited::KEY_BITS_MAX)
	                                                                  : cells_log2;
	return compact_visited::form_ok(form) ? form : 0;
}

// ---------------------------------------------------------------------------------------------------------
// Where the candidate list of a launch lives (no reference counterpart — results never depend on it):
// registers up to 512 entries (WaveList), beyond that LDS (LdsList: capacities of 513-4096 in the workgroup engine) or HBM
// (MemList: everything else — the solo shape, larger capacities, the builds).
//   list_cap     capacity of the list in memory: min(limit, rows) for limits above 512, 0 = the list is in registers
//   slot_bytes   LDS of one walker's slot WITHOUT the list (engine_slot_bytes, engine_layout.h)
//   walkers_hbm  walkers per workgroup the launch runs with the list in HBM (what it wants, bounded by what fits and by the cap)
//   walkers_cap  the ceiling on walkers per workgroup that is not a matter of LDS (option / scoring waves that must remain)
//   mode         search.list_lds: 0 never, 1 automatic — only when the workgroup keeps its walkers, so that no launch loses
//                occupancy to the list —, 2 whenever one walker fits (A/B runs, tests)
// *walkers_lds (may be null): the walkers that fit with the list in LDS when that is the answer, else 0.
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t LIST_IN_REGISTERS = 0, LIST_IN_LDS = 1, LIST_IN_HBM = 2;
constexpr uint32_t ENGINE_HEADER_BYTES_HOST = ENGINE_HEADER_BYTES; // (the name tests/lds_list_probe.cpp reads it by: the kernels' own now)
inline uint32_t engine_walkers_that_fit(uint32_t slot_bytes, uint32_t walkers_cap) {
	return std::min<uint32_t>(walkers_cap, (160u * 1024 - ENGINE_HEADER_BYTES) / std::max<uint32_t>(1, slot_bytes));
}
inline uint32_t candidate_list_placement(uint32_t mode, uint64_t list_cap, bool solo_shape, uint32_t slot_bytes, uint32_t walkers_hbm,
                                         uint32_t walkers_cap, uint32_t *walkers_lds = nullptr) {
	if (walkers_lds)
		*walkers_lds = 0;
	if (!list_cap)
		return LIST_IN_REGISTERS;
	if (mode == 0 || solo_shape || !lds_list::cells_ok(list_cap))
		return LIST_IN_HBM;
	const uint32_t fit = engine_walkers_that_fit(slot_bytes + lds_list::bytes((uint32_t)list_cap), walkers_cap);
	if (fit < 1 || (mode == 1 && fit < walkers_hbm))
		return LIST_IN_HBM;
	if (walkers_lds)
		*walkers_lds = fit;
	return LIST_IN_LDS;
}

// ---------------------------------------------------------------------------------------------------------
// Which shape of the search engine answers a launch of n queries (no reference counterpart —
// results never depend on it):
//   workgroups  k_search: persistent 1024-thread workgroups, walkers + scoring waves exchanging rows through LDS mailboxes
//   solo        k_search_solo<.., 1>: one self-scoring wave per query
//   team        k_search_solo<.., 8>: the walking wave + helper waves behind two workgroup barriers per expansion
//   crew        (round 4) not a kernel of its own: inside k_search the LAST walker of a workgroup runs the scoring waves
//               behind two workgroup barriers instead of the mailboxes — from the first expansion on when a launch has
//               at most one query per compute unit (wide rows: the one-query probe and the join chunks at 768 dims),
//               and in the drain of every larger launch
// and what the latency-bound launches touch ahead (RowTouch: lines per row in bits 0-7; ListTouch: TOUCH_LISTS).
// ---------------------------------------------------------------------------------------------------------
constexpr uint32_t LDS_BYTES_PER_CU = 160u * 1024;
struct SearchShapePolicy {
	uint32_t solo_mode = 1;           // 0 never, 1 automatic, 2 always (vss_set_search_solo)
	uint32_t solo_max_queries = 32;   // automatic: the one-wave shape up to this many queries per launch ...
	uint32_t solo_max_bytes = 32 * 1024; // ... over rows narrow enough that a level-0 list of them is within this
	bool team = true;                 // vss_set_search_team
	uint32_t n_cus = 256;             // a team wants a compute unit per query
	bool touch_rows = true, touch_lists = true;
	uint32_t touch_max_queries = 256; // touches cost bandwidth: only launches that cannot be bound by it
	bool force_looping = false;
	bool crew = true;                 // vss_set_search_crew
	uint32_t engine_walkers = 0;      // vss_set_search_params: walkers per workgroup forced (0 = from the launch size)
};
struct SearchShape {
	bool solo = false, team = false;
	uint32_t touch_lines = 0;
	bool crew = false;  // workgroup engine: the last walker of a workgroup may run its scoring waves as a crew
	bool roomy = false; // one walker per compute unit from the start: the visited set may take up to 64 KiB of LDS
};
// chunks per lane of the unrolled kernel variants (0 = the looping kernels): V float4 chunks per row over G lanes
inline uint32_t chunks_per_lane(uint64_t V, uint64_t G, bool force_looping) {
	return (V % G == 0 && !force_looping) ? (uint32_t)(V / G) : 0u;
}
// team variants exist for one chunk per lane and for the looping kernels (wide rows stay with the workgroup engine: a team
// of 8 measured slower than its 15 scoring waves, profiles/r03s_engine_shapes_by_batch_3m768_wide_rows.txt)
inline bool team_variant_exists(uint32_t nch) {
	return nch <= 1;
}
// rows of at most this many 128-byte lines are touched ahead by a team's helpers (= vss::team_touch_max_lines)
inline uint32_t team_touch_lines_max(uint32_t nch) {
	return nch > 0 ? 8 * nch : 8;
}
inline bool wants_solo(const SearchShapePolicy &p, uint32_t n, uint64_t M0, uint64_t V, uint64_t G) {
	if (p.solo_mode != 1)
		return p.solo_mode == 2;
	if (M0 * V * 16 > p.solo_max_bytes)
		return false;
	return n <= p.solo_max_queries ||
	       (p.team && team_variant_exists(chunks_per_lane(V, G, p.force_looping)) && n <= p.n_cus);
}
// the workgroup engine with ONE walker per workgroup from the start (a launch of at most one query per compute unit, or forced)
inline bool one_walker_launch(const SearchShapePolicy &p, uint32_t n) {
	return p.engine_walkers ? p.engine_walkers == 1 : n <= p.n_cus;
}
// The shape is settled in two steps, because the LDS of a solo workgroup depends on the visited set and the visited set's size
// on the shape: first everything that needs no LDS figure — solo or not (the ONE question put to wants_solo per launch), the
// roomy visited set, and for the workgroup engine the crew and its ListTouch ...
inline SearchShape search_shape_before_lds(const SearchShapePolicy &p, uint32_t n, uint64_t M0, uint64_t V, uint64_t G) {
	SearchShape s;
	s.solo = wants_solo(p, n, M0, V, G);
	if (!s.solo) {
		s.crew = p.crew;
		// a launch of at most one query per compute unit runs one walker per workgroup: alone from the first expansion on,
		// i.e. a latency chain — ListTouch as in the solo shape (a 128-byte line per accepted row; RowTouch never: the rows
		// the engine serves are wide, and pulling 64 of them ahead would swamp the compute unit's fill rate)
		const bool one_walker = s.roomy = one_walker_launch(p, n);
		if (s.crew && one_walker && n <= p.n_cus && n <= p.touch_max_queries && p.touch_lists)
			s.touch_lines = TOUCH_LISTS;
		return s;
	}
	s.roomy = true; // (one walker per compute unit, like a one-walker launch of the engine: the unit's LDS to itself)
	return s;
}
// ... then, for the solo shape only, whether it runs as a team and what it touches ahead.
// solo_lds_bytes: the dynamic LDS of one solo workgroup for this launch (visited set, staged query, id / distance buffers)
inline void settle_solo_shape(const SearchShapePolicy &p, SearchShape &s, uint32_t n, uint64_t V, uint64_t G, uint32_t solo_lds_bytes) {
	if (!s.solo)
		return;
	const uint32_t nch = chunks_per_lane(V, G, p.force_looping);
	s.team = p.team && team_variant_exists(nch) && n <= p.n_cus && solo_lds_bytes + TEAM_BOX_BYTES <= LDS_BYTES_PER_CU;
	if (n <= p.touch_max_queries) {
		const uint32_t row_lines = (uint32_t)((V * 16 + 127) / 128);
		const uint32_t max_lines = s.team ? team_touch_lines_max(nch) : 4u; // (the lone wave: RowTouch<.., 4>)
		if (p.touch_rows && row_lines <= max_lines)
			s.touch_lines = row_lines;
		if (p.touch_lists)
			s.touch_lines |= TOUCH_LISTS;
	}
}
inline SearchShape choose_search_shape(const SearchShapePolicy &p, uint32_t n, uint64_t M0, uint64_t V, uint64_t G,
                                       uint32_t solo_lds_bytes) {
	SearchShape s = search_shape_before_lds(p, n, M0, V, G);
	settle_solo_shape(p, s, n, V, G, solo_lds_bytes);
	return s;
}

// ---------------------------------------------------------------------------------------------------------
// plan_search_launch — THE one place where a launch of the search engine is decided (no reference counterpart —
// results never depend on any of it): shape, visited set, candidate list, scoring options and HBM scratch, from what the index
// and its options contribute (SearchEngineConfig) and what varies per launch (SearchLaunchInput).  Pure: the engine's
// launch_search_kernel only carries the plan out (allocations, row codes, queue words, events, the launch itself), and the CPU
// tests replay launches recorded on a GPU through it (tests/test_search_plan.py).
// ---------------------------------------------------------------------------------------------------------
struct SearchEngineConfig {
	SearchShapePolicy policy; // with it: n_cus, search.walkers (engine_walkers) and search.touch_lists (touch_lists)
	uint64_t M0 = 32, V = 1, G = 1, list_cap_max = 64;
	uint64_t nodes = 0;          // slots in use (the compact visited set's keys must cover them)
	uint32_t hash_max_log2 = 10; // a visited set of this size cannot overflow: every node fits below the 7/8 fill limit
	uint32_t search_waves = 16, search_walkers_cap = 4, search_wgs_per_cu = 1;
	uint32_t search_spec_active = 0;
	bool search_pipelined = true, search_wide_lists = true;
	uint32_t search_list_lds = 1, search_prescore = 1;
	bool search_prescore_descent = true;
	bool retry_in_place = true;
	uint64_t visited_per_limit = 0;                                 // 0 = the sizing rule's own
	uint32_t hash_lds_max_log2 = 13, hash_lds_max_override = 0;     // the LDS table ceiling with several walkers (0 = no override)
	bool visited_compact_on = true;
	uint32_t search_crew_tune = 0;
};
struct SearchLaunchInput {
	uint32_t n = 0;             // queries of this launch (all of the batch, or a retry pass's)
	uint64_t limit = 0;         // max(k, ef)
	uint32_t bump = 0, min_hash_log2 = 0; // retry passes: a larger visited set, strictly larger than the one that overflowed
	uint64_t list_cap = 0;      // capacity of the candidate list in memory, 0 = the list is in registers
	uint32_t cand_cap = 0;      // cells of the unbounded candidate queue (tomb == 2)
	uint32_t tomb = 0;          // SearchArgs::tomb
	bool direct_io = false;     // the host-pointer probe: answers straight into pinned memory
};
struct SearchLaunchPlan {
	// shape
	bool solo = false, team = false;
	uint32_t threads = 0, walkers = 0, grid = 0, lds_bytes = 0, regs = 0, nch = 0;
	// visited set
	uint32_t hash_log2 = 0;
	bool hash_in_lds = false;
	uint32_t visited_compact = 0, stage_cap = 0;
	uint32_t retry_log2 = 0; // wanted: the engine drops it when the tables cannot be allocated
	bool roomy = false;
	// candidate list
	uint32_t list_place = LIST_IN_REGISTERS, list_lds = 0;
	// scoring
	uint32_t pipelined = 0, crew = 0, touch_lines = 0, spec_active = 0;
	bool wants_prescore = false; // the engine filters where the row codes can be had
	uint32_t prescore_descent = 0; // (with the filter only)
	// scratch in HBM, in words (0 = none)
	uint64_t global_hash = 0, retry_hash = 0, list_buf = 0, cand_buf = 0;
	uint32_t shape[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // vss_last_search_shape
};
inline SearchLaunchPlan plan_search_launch(const SearchEngineConfig &e, const SearchLaunchInput &in) {
	SearchLaunchPlan a;
	const SearchShapePolicy &policy = e.policy;
	const uint32_t n = in.n, n_cus = policy.n_cus, V = (uint32_t)e.V, list_cap_max = (uint32_t)e.list_cap_max;
	SearchShape shape = search_shape_before_lds(policy, n, e.M0, e.V, e.G);
	const bool solo = a.solo = shape.solo;
	// One walker per compute unit — the solo shape, or the workgroup engine on a launch of at most one query per compute
	// unit — has the unit's LDS to itself: a visited set four times roomier (at most 64 KiB) keeps the probe sequences of
	// a chunk of 64 ids short — the gather phase is dominated by them
	const bool roomy = a.roomy = shape.roomy;
	a.hash_log2 = visited_set_log2(in.limit, in.bump, e.M0, e.list_cap_max,
	                               e.visited_per_limit ? e.visited_per_limit : search_cells_per_limit(in.limit), e.hash_max_log2);
	if (roomy && a.hash_log2 <= e.hash_lds_max_log2)
		a.hash_log2 = std::min<uint32_t>({a.hash_log2 + 2, 14u, std::max(a.hash_log2, e.hash_max_log2)});
	// a retry after a visited-set overflow must get a LARGER table than the one that overflowed, whatever shape and
	// enlargement the pass before had (min_hash_log2 = that table's size + 1; nothing exceeds "every node fits")
	a.hash_log2 = std::max(a.hash_log2, std::min(in.min_hash_log2, e.hash_max_log2));
	// LDS or HBM: tables up to 32 KiB stay in LDS (four walkers per workgroup).  (Measured and not kept: 64-KiB tables in LDS
	// with two walkers — 0.77 against 0.60 of the HBM peak at 12.5M x 1536 / ef 192, but 0.45 against 0.56 at 768 dims and
	// 0.51 against 0.63 on the configs[4] shard at ef 480: two walkers do not feed a compute unit once expansions are thin.)
	const uint32_t lds_table_log2 = roomy ? 14u : (e.hash_lds_max_override ? e.hash_lds_max_override : e.hash_lds_max_log2);
	bool hash_in_lds = a.hash_log2 <= lds_table_log2;
	// Limits of 257-512 — the 8-register list's instantiation — whose 32-bit table would go to HBM take the COMPACT exact
	// form instead (16-bit cells: tag + displacement, wave_primitives.h) over the largest table LDS admits: twice the cells
	// in the same bytes, every probe an LDS round trip instead of an L2 / memory one (2M x 1536 at ef 480 / 320: 0.52 -> 0.60
	// / 0.59 -> 0.68 of the HBM peak, answers and work counters identical: profiles/r04_compact_visited_set_*.txt).  Slots
	// must fit 24 bits; first pass only — a query that overflows it (too many visits, or a displacement beyond its bits)
	// is re-run with the plain table like any other overflow.  vss_set_search_visited_set(index, 0, ..) turns it off for A/B.
	// (the rule: compact_visited_cells_log2 above)
	a.visited_compact = e.visited_compact_on ? compact_visited_cells_log2(hash_in_lds, solo, !in.list_cap, in.limit, e.nodes,
	                                                                      !in.bump && !in.min_hash_log2, lds_table_log2)
	                                         : 0u;
	if (a.visited_compact) {
		a.hash_log2 = lds_table_log2;
		hash_in_lds = true;
	}
	a.hash_in_lds = hash_in_lds;
	// walkers per workgroup: as many as the batch needs to cover every compute unit once, as many as LDS admits
	uint32_t waves = std::max<uint32_t>(2, std::min<uint32_t>(e.search_waves, 16));
	// the accept phase of an expansion in the shadow of the successor's row loads (level_search_pipelined): plain searches
	// with a register list over neighbour lists of at most 64 cells.  Limits of 257-512 (the 8-register list) are pipelined
	// in 12-wave workgroups only (170 registers per lane: k_search<.., WIDE_LIST_THREADS>, round 5) — four walkers and eight
	// scoring waves; vss_set_search_wide_lists(0) keeps them in 16 waves and the plain order (round 4; A/B)
	const bool wide_limit = in.limit > 64u * PIPELINED_MAX_REGS; // (beyond the 4-register list: walker-bound, two waves per walker)
	const bool can_pipeline = e.search_pipelined && !solo && !in.tomb && !in.list_cap && list_cap_max <= 64;
	const bool wide_list = can_pipeline && e.search_wide_lists && wide_limit;
	if (wide_list)
		waves = std::min<uint32_t>(waves, WIDE_LIST_THREADS / 64);
	a.pipelined = (can_pipeline && (wide_list || !wide_limit)) ? 1u : 0u;
	// (rounds 2-5 staged the batched list merge here — `limit` cells per walker; the blocked list of round 6 merges nothing.
	//  What is left is four words per walker of the 8-register list's kernels: where its visited set moves when it outgrows
	//  LDS, WaveLds::spill_box)
	const bool wide_register_list = !solo && !in.list_cap && wide_limit; // (k_search<.., 8, ..>)
	a.stage_cap = wide_register_list ? 4u : 0u;
	const uint32_t slot_bytes = engine_slot_bytes(a.hash_log2, V, list_cap_max, hash_in_lds, a.stage_cap);
	const uint32_t walkers_cap = std::min<uint32_t>(policy.engine_walkers ? ENGINE_MAX_WALKERS : e.search_walkers_cap, waves - 1);
	uint32_t S = policy.engine_walkers ? policy.engine_walkers : (n + n_cus - 1) / n_cus;
	S = std::max<uint32_t>(1, std::min(S, engine_walkers_that_fit(slot_bytes, walkers_cap)));
	// Limits beyond the register lists: the candidate list in the walkers' slots of LDS (capacities of 513-4096; LdsList) where
	// the workgroup keeps the walkers it has with the list in HBM — no launch loses occupancy to it —, else in HBM as before
	// (the rule: candidate_list_placement above; search.list_lds = 0 is the path without it, exactly).  Retry passes come
	// through here like every launch.
	uint32_t walkers_lds = 0;
	a.list_place = candidate_list_placement(e.search_list_lds, in.list_cap, solo, slot_bytes, S, walkers_cap, &walkers_lds);
	const bool list_in_lds = a.list_place == LIST_IN_LDS;
	a.list_lds = list_in_lds ? (uint32_t)in.list_cap : 0u;
	if (list_in_lds)
		S = std::min(S, walkers_lds); // (search.list_lds = 2 only: the automatic rule never takes a walker away)
	const auto engine_lds = [&](uint32_t walkers) {
		return engine_lds_bytes(walkers, a.hash_log2, V, list_cap_max, hash_in_lds, a.stage_cap, a.list_lds);
	};
	// workgroups per compute unit: one 16-wave workgroup — or, with fewer waves per workgroup (vss_set_search_params), as
	// many as the waves and the LDS admit, so that a workgroup of the NEXT launch can move in beside one that still drains
	// (VSS_SEARCH_WGS_PER_CU caps it, default 1.  Measured: two 8-wave workgroups of 2 walkers + 6 scoring waves per compute
	// unit run every regime at the rate of one 16-wave workgroup of 4 + 12 — profiles/r04_two_workgroups_per_compute_unit_no_gain.txt)
	uint32_t wgs_per_cu = std::max<uint32_t>(1, std::min<uint32_t>(16u / waves, LDS_BYTES_PER_CU / std::max<uint32_t>(1, engine_lds(S))));
	wgs_per_cu = std::min(wgs_per_cu, e.search_wgs_per_cu);
	uint32_t grid = std::min<uint32_t>(n_cus * wgs_per_cu, (n + S - 1) / S);
	const uint32_t solo_lds = wave_lds_bytes(a.hash_log2, V, list_cap_max, a.stage_cap, hash_in_lds);
	if (solo) { // one single-wave workgroup per query in flight, as many per compute unit as LDS admits (at most 8)
		S = 1;
		grid = std::min<uint32_t>(n, n_cus * std::max<uint32_t>(1, std::min<uint32_t>(8, LDS_BYTES_PER_CU / solo_lds)));
	}
	// a query that outgrows its LDS-resident set is repeated by its walker, in the same launch, over a table in HBM (2^17
	// cells = 512 KiB per walker, or what holds the whole index if that is less) — where overflows are a per-cent matter:
	// limits of 257-512, the compact form (the only instantiations that carry the code: k_search<.., 8, ..>)
	if (e.retry_in_place && wide_register_list && hash_in_lds) {
		const uint32_t have_log2 = a.visited_compact ? compact_visited::cells_log2_of(a.visited_compact) : a.hash_log2;
		const uint32_t want_log2 = std::min<uint32_t>(17u, e.hash_max_log2);
		if (want_log2 > have_log2)
			a.retry_log2 = want_log2;
	}
	// scratch in HBM scales with the resident walkers: bound it (retry passes with very large tables run fewer at a time)
	// (the retry tables count: ADVICE r05 — 512 MiB per context that runs such limits went unbudgeted)
	const uint64_t per_walker = (hash_in_lds ? 0 : (4ull << a.hash_log2)) + (list_in_lds ? 0 : 8ull * in.list_cap) +
	                            (in.tomb == 2 ? 8ull * in.cand_cap : 0) + (a.retry_log2 ? (4ull << a.retry_log2) : 0);
	const uint64_t budget = 16ull << 30;
	while (per_walker * grid * S > budget && (grid > 1 || S > 1)) {
		if (S > 1)
			S--;
		else
			grid = (grid + 1) / 2;
	}
	a.walkers = S;
	a.grid = grid;
	const uint64_t resident = (uint64_t)grid * S;
	a.global_hash = hash_in_lds ? 0 : resident << a.hash_log2;
	a.retry_hash = a.retry_log2 ? resident << a.retry_log2 : 0;
	a.list_buf = (in.list_cap && !list_in_lds) ? resident * 2 * in.list_cap : 0;
	a.cand_buf = in.tomb == 2 ? resident * 2 * in.cand_cap : 0;
	// one expansion of look-ahead while scoring waves are idle (lists of at most 64 cells: one cell per lane)
	a.spec_active = (!in.tomb && !solo && list_cap_max <= 64) ? e.search_spec_active : 0;
	// latency-bound launches of the solo shape (at most one query per compute unit): pull the rows the cached lists name
	// (RowTouch: by the team's helpers, or by the lone wave for rows of at most four 128-byte lines) and the lists of the
	// rows being accepted (ListTouch) into L2 ahead of time.  Costs bandwidth, so never for launches that could be bound by it.
	// A team (helper waves on the compute unit's other SIMDs score a share of every expansion's rows) while every query
	// of the launch still gets a compute unit of its own; its job box takes the first bytes of the workgroup's LDS
	settle_solo_shape(policy, shape, n, e.V, e.G, solo_lds);
	a.team = shape.team;
	a.touch_lines = shape.touch_lines;
	// the last walker of a workgroup runs its scoring waves as a crew (two barriers per expansion instead of the mailbox
	// exchange): from the start when S = 1, in the drain of a larger launch otherwise
	a.crew = shape.crew ? (CREW_ON | ((policy.touch_lists && list_cap_max <= 64) ? CREW_TOUCH : 0u) | e.search_crew_tune) : 0u;
	// pre-scoring on row codes (search.prescore): the pipelined level search over the mailbox exchange only; the pinned
	// small-batch probe (latency-bound: crews) is left alone.  Limits above 256 only when asked for (search.prescore = 2)
	a.wants_prescore = a.pipelined && !in.direct_io && (e.search_prescore == 2 || !wide_limit);
	// (the same launches, no others: without codes the kernel ignores it)
	a.prescore_descent = (a.wants_prescore && e.search_prescore_descent) ? 1u : 0u;
	a.nch = chunks_per_lane(e.V, e.G, policy.force_looping);
	a.regs = (uint32_t)((in.limit + 63) / 64);
	a.lds_bytes = solo ? solo_lds + (a.team ? TEAM_BOX_BYTES : 0u) : engine_lds(S);
	a.threads = solo ? (a.team ? 64 * VSS_TEAM_WAVES : 64) : 64 * waves;
	const uint32_t words[8] = {a.threads, S, grid, a.lds_bytes, a.list_place, hash_in_lds ? (a.visited_compact ? 1u : 0u) : 2u,
	                           solo ? 1u : 0u, 0u};
	std::copy(words, words + 8, a.shape);
	return a;
}

} // namespace host
} // namespace vss
