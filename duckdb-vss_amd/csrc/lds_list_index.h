// lds_list_index.h — the index arithmetic of the candidate list kept in LDS (wave_primitives.h: LdsList), shared by the device
// code, the host (engine_layout.h: the bytes a walker's slot sets aside for it; host_logic.h: when a launch takes it) and
// tests/lds_list_probe.cpp: a lane-by-lane model of the list checked against std::vector on the CPU.  No reference counterpart:
// usearch's sorted_buffer_gt (index.hpp:783-917) is one array searched by bisection.
//
// The list is two plain arrays of `cells` words — distances ascending, slots — cut into tiles of 64 entries (one per lane), plus
// a compact array of TILE TOPS: tops[t] = the distance at position 64 t + 63, kept for every tile whose last position has been
// written.  lower_bound reads the tops with one cell per lane (64 consecutive words: no bank conflict; reading "every 64th
// distance" instead would hit one bank 64 times), counts the full tiles that lie wholly below the new distance, and ballots
// over the one tile after them: two dependent LDS reads whatever the size.  A top changes exactly when position 64 t + 63 is
// written — by the shift (the entry coming up from 64 t + 62) or by the new entry itself — and the lane that writes the
// position writes the top.
#pragma once
#include <stdint.h>

#include "visited_compact.h" // VSS_HD

namespace vss {
namespace lds_list {

constexpr uint32_t TILE = 64;
constexpr uint32_t MIN_CELLS = 513;  // smaller lists live in registers (WaveList: 64 * MAX_LIST_REGS entries)
constexpr uint32_t MAX_CELLS = 4096; // 64 tiles: their tops are one cell per lane
constexpr uint32_t TOP_CELLS = MAX_CELLS / TILE;

VSS_HD uint32_t align16(uint32_t x) {
	return (x + 15u) & ~15u;
}
// bytes of a walker's slot taken by a list of `cells` entries (0 = no list in LDS): distances, slots, tile tops
VSS_HD uint32_t bytes(uint32_t cells) {
	return cells ? 2 * align16(4 * cells) + 4 * TOP_CELLS : 0;
}
VSS_HD bool cells_ok(uint64_t cells) {
	return cells >= MIN_CELLS && cells <= MAX_CELLS;
}
// tiles of a list of `size` entries whose top is kept (the full ones)
VSS_HD int full_tiles(int size) {
	return size >> 6;
}
// the tile whose top lives at `pos`, or -1
VSS_HD int top_at(int pos) {
	return (pos & 63) == 63 ? pos >> 6 : -1;
}
// `below`: bit t = "tile t is full and its top is < the new distance".  The tiles that lie wholly below it are the leading
// ones (the list is sorted) — counted as the run of set bits from bit 0, which is where a tile-by-tile walk would stop.
VSS_HD int tiles_below(unsigned long long below) {
	return ~below ? __builtin_ctzll(~below) : 64;
}
// one step of the shift of [p, hi) one cell up, highest tile first: the entries [lo, hi) move, then hi = lo
VSS_HD int shift_window_lo(int p, int hi) {
	const int lo = (hi - 1) & ~63;
	return lo < p ? p : lo;
}

} // namespace lds_list
} // namespace vss
