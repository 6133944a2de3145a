// host_logic_probe.cpp — C surface over duckdb-vss_amd/csrc/host_logic.h (the engine's pure host logic) for the CPU tests
// in tests/test_host_logic.py.  Built with plain g++: nothing here needs HIP or a GPU.
#include <cstring>

#include "../duckdb-vss_amd/csrc/host_logic.h"

using namespace vss::host;

extern "C" {

// the first n levels the engine draws for connectivity M after a reserve (stage_metadata)
void hl_draw_levels(uint64_t M, uint64_t n, uint8_t *out) {
	LevelRng rng;
	const double inv = inverse_log_connectivity(M);
	for (uint64_t i = 0; i != n; ++i)
		out[i] = rng.stored_level(inv);
}

uint64_t hl_schedule(uint64_t existing, int max_level, const uint8_t *levels, uint64_t n, uint64_t max_batch,
                     uint64_t growth_div, int64_t solo_row, uint64_t *out_sizes) {
	auto s = batch_schedule(existing, max_level, levels, n, max_batch, growth_div, solo_row < 0 ? ~0ull : (uint64_t)solo_row);
	for (size_t i = 0; i != s.size(); ++i)
		out_sizes[i] = s[i];
	return s.size();
}

// Replays a script on the free ring exactly as the engine drives it: op > 0 = remove() of slot op-1 (reserve(size()+1) +
// push), op == 0 = one add() asking for a slot (try_pop).  out[i] = the slot an add received, or -1 (append), or -2 for
// remove ops.
void hl_ring_script(const int64_t *ops, uint64_t n, int64_t *out) {
	FreeRing ring;
	for (uint64_t i = 0; i != n; ++i) {
		if (ops[i] > 0) {
			ring.reserve(ring.size() + 1);
			ring.push((uint32_t)(ops[i] - 1));
			out[i] = -2;
		} else {
			uint32_t s = NO_SLOT;
			out[i] = ring.try_pop(s) ? (int64_t)s : -1;
		}
	}
}

// KeyMap: put keys[i] -> i, erase the flagged ones, look everything up again; returns the number of mismatches
uint64_t hl_keymap_check(const int64_t *keys, const uint8_t *erase, uint64_t n) {
	KeyMap m;
	m.init(4);
	for (uint64_t i = 0; i != n; ++i)
		m.put(keys[i], (uint32_t)i);
	for (uint64_t i = 0; i != n; ++i)
		if (erase[i])
			m.erase(keys[i]);
	uint64_t bad = 0;
	for (uint64_t i = 0; i != n; ++i) {
		uint32_t s = NO_SLOT;
		const bool found = m.find(keys[i], s);
		bad += erase[i] ? found : (!found || s != (uint32_t)i);
	}
	uint32_t s;
	bad += m.find(-12345, s);
	return bad;
}

// choose_search_shape over the engine's default policy with the given overrides;
// out = {solo, team, touch_lines, wants_solo, crew, roomy}
void hl_search_shape(uint32_t n, uint64_t M0, uint64_t V, uint64_t G, uint32_t solo_lds_bytes, uint32_t solo_mode, int team,
                     int touch_rows, int touch_lists, uint32_t n_cus, int force_looping, int crew, uint32_t engine_walkers,
                     uint32_t *out) {
	SearchShapePolicy p;
	p.solo_mode = solo_mode, p.team = team != 0, p.touch_rows = touch_rows != 0, p.touch_lists = touch_lists != 0;
	p.n_cus = n_cus, p.force_looping = force_looping != 0;
	p.crew = crew != 0, p.engine_walkers = engine_walkers;
	const SearchShape s = choose_search_shape(p, n, M0, V, G, solo_lds_bytes);
	out[0] = s.solo, out[1] = s.team, out[2] = s.touch_lines;
	out[3] = wants_solo(p, n, M0, V, G);
	out[4] = s.crew, out[5] = s.roomy;
}

// plan_search_launch over flat arrays (tests/test_search_plan.py names the cells in this order):
//   cfg  solo_mode, solo_max_queries, solo_max_bytes, team, n_cus, touch_rows, touch_lists, touch_max_queries, force_looping, crew,
//        engine_walkers, M0, V, G, list_cap_max, nodes, hash_max_log2, search_waves, search_walkers_cap, search_wgs_per_cu,
//        search_spec_active, search_pipelined, search_wide_lists, search_list_lds, search_prescore, search_prescore_descent,
//        retry_in_place, visited_per_limit, hash_lds_max_log2, hash_lds_max_override, visited_compact_on, search_crew_tune
//   in   n, limit, bump, min_hash_log2, list_cap, cand_cap, tomb, direct_io
//   out  solo, team, threads, walkers, grid, lds_bytes, regs, nch, hash_log2, hash_in_lds, visited_compact, stage_cap, retry_log2,
//        roomy, list_place, list_lds, pipelined, crew, touch_lines, spec_active, wants_prescore, prescore_descent, global_hash,
//        retry_hash, list_buf, cand_buf, shape[0..8)
void hl_plan_search_launch(const uint64_t *cfg, const uint64_t *in, uint64_t *out) {
	SearchEngineConfig e;
	SearchShapePolicy &p = e.policy;
	int i = 0;
	p.solo_mode = (uint32_t)cfg[i++], p.solo_max_queries = (uint32_t)cfg[i++], p.solo_max_bytes = (uint32_t)cfg[i++];
	p.team = cfg[i++] != 0, p.n_cus = (uint32_t)cfg[i++], p.touch_rows = cfg[i++] != 0, p.touch_lists = cfg[i++] != 0;
	p.touch_max_queries = (uint32_t)cfg[i++], p.force_looping = cfg[i++] != 0, p.crew = cfg[i++] != 0;
	p.engine_walkers = (uint32_t)cfg[i++];
	e.M0 = cfg[i++], e.V = cfg[i++], e.G = cfg[i++], e.list_cap_max = cfg[i++], e.nodes = cfg[i++];
	e.hash_max_log2 = (uint32_t)cfg[i++], e.search_waves = (uint32_t)cfg[i++], e.search_walkers_cap = (uint32_t)cfg[i++];
	e.search_wgs_per_cu = (uint32_t)cfg[i++], e.search_spec_active = (uint32_t)cfg[i++], e.search_pipelined = cfg[i++] != 0;
	e.search_wide_lists = cfg[i++] != 0, e.search_list_lds = (uint32_t)cfg[i++], e.search_prescore = (uint32_t)cfg[i++];
	e.search_prescore_descent = cfg[i++] != 0, e.retry_in_place = cfg[i++] != 0, e.visited_per_limit = cfg[i++];
	e.hash_lds_max_log2 = (uint32_t)cfg[i++], e.hash_lds_max_override = (uint32_t)cfg[i++], e.visited_compact_on = cfg[i++] != 0;
	e.search_crew_tune = (uint32_t)cfg[i++];
	SearchLaunchInput l;
	l.n = (uint32_t)in[0], l.limit = in[1], l.bump = (uint32_t)in[2], l.min_hash_log2 = (uint32_t)in[3], l.list_cap = in[4];
	l.cand_cap = (uint32_t)in[5], l.tomb = (uint32_t)in[6], l.direct_io = in[7] != 0;
	const SearchLaunchPlan a = plan_search_launch(e, l);
	const uint64_t flat[] = {a.solo, a.team, a.threads, a.walkers, a.grid, a.lds_bytes, a.regs, a.nch, a.hash_log2, a.hash_in_lds,
	                         a.visited_compact, a.stage_cap, a.retry_log2, a.roomy, a.list_place, a.list_lds, a.pipelined, a.crew,
	                         a.touch_lines, a.spec_active, a.wants_prescore, a.prescore_descent, a.global_hash, a.retry_hash,
	                         a.list_buf, a.cand_buf};
	std::memcpy(out, flat, sizeof flat);
	for (int w = 0; w != 8; ++w)
		out[sizeof flat / sizeof flat[0] + w] = a.shape[w];
}

// visited-set sizing of a SEARCH with this limit (cells per limit entry chosen by search_cells_per_limit)
uint32_t hl_search_visited_log2(uint64_t limit, uint32_t bump, uint64_t M0, uint64_t list_cap_max, uint32_t max_log2) {
	return visited_set_log2(limit, bump, M0, list_cap_max, search_cells_per_limit(limit), max_log2);
}
// when a launch takes the compact visited set, and with how many cells (0 = the plain 32-bit set)
uint32_t hl_compact_cells_log2(int plain_fits_lds, int solo, int register_list, uint64_t limit, uint64_t nodes, int first_pass,
                               uint32_t lds_table_log2) {
	return compact_visited_cells_log2(plain_fits_lds != 0, solo != 0, register_list != 0, limit, nodes, first_pass != 0, lds_table_log2);
}
// A sequential model of the compact set over visited_compact.h's arithmetic (the device code runs the same probe sequence with
// a compare-and-swap per cell): out[i] = 1 if keys[i] was present, 0 if it was inserted now, 2 if it could not be placed
// (displacement beyond its bits).  Returns the number of cells in use.
uint64_t hl_compact_model(const uint32_t *keys, uint64_t n, uint32_t cells_log2, uint8_t *out) { // (cells_log2: the set's FORM)
	const uint32_t cells = 1u << vss::compact_visited::cells_log2_of(cells_log2);
	std::vector<uint16_t> table((size_t)cells, (uint16_t)vss::compact_visited::EMPTY16);
	const uint32_t mask = cells - 1;
	uint64_t used = 0;
	for (uint64_t i = 0; i != n; ++i) {
		uint32_t c, want;
		out[i] = 2;
		for (vss::compact_visited::home_of(keys[i], cells_log2, c, want); !vss::compact_visited::placed_too_far(want, cells_log2);
		     c = (c + 1) & mask, ++want) {
			if (table[c] == want) {
				out[i] = 1;
				break;
			}
			if (table[c] == vss::compact_visited::EMPTY16) {
				table[c] = (uint16_t)want;
				out[i] = 0;
				++used;
				break;
			}
		}
	}
	return used;
}
// (home cell, tag) of a key: distinct keys below 2^24 must never share both
void hl_compact_home(const uint32_t *keys, uint64_t n, uint32_t cells_log2, uint32_t *cells, uint32_t *tags) {
	for (uint64_t i = 0; i != n; ++i) {
		uint32_t c, want;
		vss::compact_visited::home_of(keys[i], cells_log2, c, want);
		cells[i] = c;
		tags[i] = want >> (16 - vss::compact_visited::tag_bits(cells_log2));
	}
}
// ... and of the build's insert search (always 64 cells per entry)
uint32_t hl_build_visited_log2(uint64_t limit, uint32_t bump, uint64_t M0, uint64_t list_cap_max, uint32_t max_log2) {
	return visited_set_log2(limit, bump, M0, list_cap_max, 64, max_log2);
}
}
