// lds_list_probe.cpp — C surface for tests/test_lds_list_logic.py over the host-side pieces of the candidate list in LDS:
// the placement rule (duckdb-vss_amd/csrc/host_logic.h) and a lane-by-lane model of the list (the index arithmetic of
// duckdb-vss_amd/csrc/lds_list_index.h, driven the way wave_primitives.h LdsList drives it) checked against std::vector.
// Built with plain g++: nothing here needs HIP or a GPU.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../duckdb-vss_amd/csrc/host_logic.h"
#include "../duckdb-vss_amd/csrc/lds_list_index.h"

using namespace vss;

namespace {

// LdsList, one loop iteration per lane: every "instruction" reads with all lanes before any lane writes
struct Model {
	std::vector<float> d, tops;
	std::vector<uint32_t> s;
	int size = 0, limit = 0;
	uint64_t reads = 0; // dependent LDS reads of the last lower_bound
	Model(int cells, int lim) : d(cells, -1.f), tops(lds_list::TOP_CELLS, -2.f), s(cells, 0), limit(lim) {
	}
	int lower_bound(float nd) {
		unsigned long long below = 0;
		const int full = lds_list::full_tiles(size);
		for (int lane = 0; lane < 64; ++lane)
			if (lane < full && tops[lane] < nd)
				below |= 1ull << lane;
		reads = 1;
		const int base = 64 * lds_list::tiles_below(below);
		if (base >= size)
			return base;
		int c = 0;
		for (int lane = 0; lane < 64; ++lane)
			c += base + lane < size && d[base + lane] < nd;
		reads = 2;
		return base + c;
	}
	bool insert(float nd, uint32_t ns) {
		const int p = lower_bound(nd);
		if (p == limit)
			return false;
		for (int hi = size < limit ? size : limit - 1; hi > p;) {
			const int lo = lds_list::shift_window_lo(p, hi);
			float vd[64];
			uint32_t vs[64];
			for (int lane = 0; lane < 64; ++lane)
				if (lo + lane < hi)
					vd[lane] = d[lo + lane], vs[lane] = s[lo + lane];
			for (int lane = 0; lane < 64; ++lane)
				if (lo + lane < hi) {
					const int to = lo + lane + 1;
					d.at(to) = vd[lane], s.at(to) = vs[lane];
					if (lds_list::top_at(to) >= 0)
						tops.at(lds_list::top_at(to)) = vd[lane];
				}
			hi = lo;
		}
		d.at(p) = nd, s.at(p) = ns;
		if (lds_list::top_at(p) >= 0)
			tops.at(lds_list::top_at(p)) = nd;
		if (size < limit)
			size++;
		return true;
	}
};

} // namespace

extern "C" {

uint32_t ll_placement(uint32_t mode, uint64_t list_cap, int solo, uint32_t slot_bytes, uint32_t walkers_hbm, uint32_t walkers_cap,
                      uint32_t *walkers_lds) {
	return host::candidate_list_placement(mode, list_cap, solo != 0, slot_bytes, walkers_hbm, walkers_cap, walkers_lds);
}
uint32_t ll_engine_walkers_that_fit(uint32_t slot_bytes, uint32_t walkers_cap) {
	return host::engine_walkers_that_fit(slot_bytes, walkers_cap);
}
uint32_t ll_header_bytes() {
	return host::ENGINE_HEADER_BYTES_HOST;
}
uint32_t ll_list_bytes(uint32_t cells) {
	return lds_list::bytes(cells);
}

// Inserts n (distance, slot) pairs into the model and into a std::vector kept by sorted_buffer_gt's rule (before equal
// distances, bounded by `limit`, the last entry dropped when full); compares after every insert.  0 = equal throughout,
// else 1 + the index of the first insert after which they differ (or whose return value / read count is wrong).
uint64_t ll_model_check(const float *dist, const uint32_t *slot, uint64_t n, uint32_t cells, uint32_t limit) {
	Model m((int)cells, (int)limit);
	std::vector<std::pair<float, uint32_t>> want;
	for (uint64_t i = 0; i != n; ++i) {
		size_t p = 0;
		while (p < want.size() && want[p].first < dist[i])
			p++;
		const bool fits = p < limit;
		if (fits) {
			want.insert(want.begin() + p, {dist[i], slot[i]});
			if (want.size() > limit)
				want.pop_back();
		}
		if (m.insert(dist[i], slot[i]) != fits || m.reads > 2 || m.size != (int)want.size())
			return i + 1;
		for (size_t j = 0; j != want.size(); ++j)
			if (std::memcmp(&m.d[j], &want[j].first, 4) || m.s[j] != want[j].second)
				return i + 1;
		for (int t = 0; t < lds_list::full_tiles(m.size); ++t)
			if (std::memcmp(&m.tops[t], &m.d[64 * t + 63], 4))
				return i + 1;
	}
	return 0;
}
}
