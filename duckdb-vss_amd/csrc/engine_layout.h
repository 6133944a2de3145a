// engine_layout.h — the constants and LDS size formulas that the kernels (hnsw_kernels.h, wave_primitives.h) and the host's
// launch planner (host_logic.h: plan_search_launch) share.  Plain integer arithmetic, no HIP: the planner and its CPU tests
// (tests/host_logic_probe.cpp) compile the very definitions the device code is built from, so nothing is restated by hand.
#pragma once
#include <stdint.h>

#include "lds_list_index.h"
#include "visited_compact.h" // VSS_HD

namespace vss {

constexpr int MAX_LIST_REGS = 8; // 64 * 8 = 512 entries: the largest ef / ef_construction a register list holds
static_assert(lds_list::MIN_CELLS == 64 * MAX_LIST_REGS + 1, "the LDS list starts where the register lists end");

constexpr uint32_t CREW_ON = 1u, CREW_TOUCH = 2u, CREW_SPARE_SIMD = 4u, CREW_NO_REQUESTS = 8u; // SearchArgs::crew
constexpr uint32_t TOUCH_LISTS = 0x100u; // WaveLds::touch_lines / SearchArgs::touch_lines: bits 0-7 row lines, bit 8 ListTouch
struct TeamBox {
	int n;     // rows on offer (lds.ids[0..n)), < 0 = the walk is over
	float qa2; // the query's squared norm (cosine)
	uint32_t touch_n; // neighbour lists in `cells` whose rows the helpers pull into L2 after the second barrier (RowTouch)
	uint32_t pad;
	uint32_t cells[2][64];
};
constexpr uint32_t TEAM_BOX_BYTES = (uint32_t)sizeof(TeamBox); // the first bytes of a team's LDS (multiple of 16)

#ifndef VSS_TEAM_WAVES_N
#define VSS_TEAM_WAVES_N 8 // (4 and 16 measured: A/B builds)
#endif
constexpr int VSS_TEAM_WAVES = VSS_TEAM_WAVES_N; // waves per query of the solo shape's team variant (hnsw_kernels.h, TeamScorer)

// LDS header of the search engine (k_search)
constexpr uint32_t ENGINE_MAX_WALKERS = 8; // (the host keeps to 4 unless told otherwise: vss_engine.hip search_walkers_cap)
// {exit flag, walkers left, pad} + crew box + mailboxes + 64 scrap cells (the dummy targets of pool_score's all-lane atomics)
constexpr uint32_t ENGINE_BOXES = 2 * ENGINE_MAX_WALKERS; // two job buffers (and mailboxes) per walker
constexpr uint32_t ENGINE_CREW_OFFSET = 16;                       // the crew box (16 bytes) follows {exit flag, walkers left, pad}
constexpr uint32_t ENGINE_SIMD_OFFSET = 32;                       // which SIMD each of the (at most 16) waves runs on, one byte each
constexpr uint32_t ENGINE_BOX_OFFSET = 48;                        // the mailboxes
constexpr uint32_t ENGINE_SCRAP_OFFSET = ENGINE_BOX_OFFSET + ENGINE_BOXES * 32;
constexpr uint32_t ENGINE_HEADER_BYTES = ENGINE_SCRAP_OFFSET + 64 * 8;

constexpr int PIPELINED_MAX_REGS = 4; // level_search_pipelined: candidate lists of at most this many registers (limit <= 256) ...
// ... in a 1024-thread workgroup (128 registers per lane).  Round 5: limits of 257-512 — the 8-register list — run as
// 768-thread workgroups (12 waves: 170 registers per lane), where the pipeline's state fits next to the list; four walkers
// and eight scoring waves, which is plenty for expansions that bring four to eight new rows.
constexpr int WIDE_LIST_THREADS = 768;
VSS_HD constexpr int pipelined_max_regs(int workgroup_threads) {
	return workgroup_threads <= WIDE_LIST_THREADS ? MAX_LIST_REGS : PIPELINED_MAX_REGS;
}

using lds_list::align16;

// dynamic LDS bytes of one wave of the BUILD kernels (shared by host launch code and the kernels)
VSS_HD uint32_t wave_lds_bytes(uint32_t hash_log2, uint32_t V, uint32_t list_cap_max,
                               uint32_t cand_cap, bool hash_in_lds = true) {
	uint32_t b = 0;
	if (hash_in_lds)
		b += align16((1u << hash_log2) * 4);
	b += align16(V * 16) * 2;
	b += align16(list_cap_max * 4) * 2;
	b += align16(cand_cap * 4) * 2;
	b += align16((list_cap_max + 1) * 4) * 2;
	return b;
}

// LDS of the search engine: a header {exit flag, walkers still running}, S mailboxes, then per walker
// [visited set unless in HBM][staged query][ids][distances].
// stage_cap: cells of the list-merge staging area (>= the search limit for register lists, 0 = none)
// list_cells: cells of the candidate list kept in LDS (LdsList: two arrays of align16(4 x cells) bytes and the tile tops,
// lds_list_index.h), 0 = no list here.  The slot stride is computed by the host, the walker, the scoring waves' loop and
// crew_help: all four pass the same value.
VSS_HD uint32_t engine_slot_bytes(uint32_t hash_log2, uint32_t V, uint32_t list_cap_max, bool hash_in_lds,
                                  uint32_t stage_cap, uint32_t list_cells = 0) {
	return (hash_in_lds ? align16((1u << hash_log2) * 4) : 0) + align16(V * 16) + 4 * align16(list_cap_max * 4) +
	       2 * align16(stage_cap * 4) + lds_list::bytes(list_cells);
}
VSS_HD uint32_t engine_lds_bytes(uint32_t walkers, uint32_t hash_log2, uint32_t V, uint32_t list_cap_max,
                                 bool hash_in_lds, uint32_t stage_cap, uint32_t list_cells = 0) {
	return ENGINE_HEADER_BYTES + walkers * engine_slot_bytes(hash_log2, V, list_cap_max, hash_in_lds, stage_cap, list_cells);
}

} // namespace vss
