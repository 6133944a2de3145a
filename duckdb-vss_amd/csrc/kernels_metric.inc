// kernels_metric.inc — instantiates every (chunks-per-lane, rows-in-flight, list-registers) variant of the templated
// kernels for ONE metric (VSS_MT) and defines their launchers.  Included by kernels_{l2sq,cosine,ip}.hip.
#include "launchers.h"

namespace vss {

#include "launch_macros.inc"

// The search engine: c.threads / 64 waves per workgroup (walkers + scoring waves), 4 rows in flight per scoring pass
// (<= 128 VGPRs, so that a 1024-thread workgroup fits a compute unit).  The candidate list takes 2, 4 or 8 registers per
// lane, or lives in LDS (E = LDS_LIST_E: capacities of 513-4096) or in HBM (E = 0) for ef_search / k beyond 512.
// launches with one predicate per query (GraphView::filter_bits carries FILTER_PER_QUERY): the *_groups kernels, same ladders
// (such a launch is never pipelined: no 12-wave variant)
template <int MT, int NCH, int R>
static hipError_t search_groups_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.list_lds)
		VSS_LAUNCH_T((k_search_groups<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search_groups<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search_groups<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search_groups<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search_groups<MT, NCH, RS, 0>), a, c.threads);
}
// launches with one wanted label per query (filter_bits carries FILTER_BY_LABEL too): the *_labels kernels, the same ladders
template <int MT, int NCH, int R>
static hipError_t search_labels_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.list_lds)
		VSS_LAUNCH_T((k_search_labels<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search_labels<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search_labels<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search_labels<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search_labels<MT, NCH, RS, 0>), a, c.threads);
}
// launches with one label range per query (filter_bits carries FILTER_BY_RANGE instead): the *_ranges kernels, the same ladders
template <int MT, int NCH, int R>
static hipError_t search_ranges_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.list_lds)
		VSS_LAUNCH_T((k_search_ranges<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search_ranges<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search_ranges<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search_ranges<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search_ranges<MT, NCH, RS, 0>), a, c.threads);
}
// launches with one label set per query (filter_bits carries FILTER_BY_SET instead): the *_sets kernels, the same ladders
template <int MT, int NCH, int R>
static hipError_t search_sets_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.list_lds)
		VSS_LAUNCH_T((k_search_sets<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search_sets<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search_sets<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search_sets<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search_sets<MT, NCH, RS, 0>), a, c.threads);
}
template <int MT, int NCH, int R>
static hipError_t search_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.gv.filter_bits & FILTER_BY_SET)
		return search_sets_e<MT, NCH, R>(a, c);
	if (a.gv.filter_bits & FILTER_BY_RANGE)
		return search_ranges_e<MT, NCH, R>(a, c);
	if (a.gv.filter_bits & FILTER_BY_LABEL)
		return search_labels_e<MT, NCH, R>(a, c);
	if (a.gv.filter_bits & FILTER_PER_QUERY)
		return search_groups_e<MT, NCH, R>(a, c);
	// limits of 257-512, pipelined: 12-wave workgroups (170 registers per lane; 4 rows in flight at every row width)
	if (c.threads <= WIDE_LIST_THREADS && c.regs > PIPELINED_MAX_REGS && c.regs <= MAX_LIST_REGS && a.pipelined)
		VSS_LAUNCH_T((k_search<MT, NCH, 4, MAX_LIST_REGS, WIDE_LIST_THREADS>), a, c.threads);
	// capacities of 513-4096 with the list in the walkers' slots of LDS (the host's placement rule: host_logic.h)
	if (a.list_lds)
		VSS_LAUNCH_T((k_search<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search<MT, NCH, RS, 0>), a, c.threads);
}
// The solo shape (one wave per query, the walker scores its own rows): RS register slots of rows in flight, sized so that a
// whole level-0 list is one pass where the rows are narrow (16 slots x 2 rows at dimension 128) and the row window stays
// within ~200 registers where they are wide.  The list may also take a single register (limit <= 64).
// Teams (c.threads = 64 x VSS_TEAM_WAVES: the helpers share every expansion's rows) exist for the narrow-row variants the
// solo shape is chosen for — one chunk per lane, and the looping kernels.  For wide rows (768 dims) a team of 8 measured
// SLOWER than the workgroup engine's 15 scoring waves up to 128 queries per launch (profiles/r03s_*_wide_rows.txt), and 16
// waves of this kernel do not fit the register file.
template <int MT, int NCH>
static hipError_t search_team_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int T = VSS_TEAM_WAVES, RT = VSS_TEAM_R;
	if (a.gv.filter_bits & FILTER_BY_SET) {
		if (c.regs <= 1)
			VSS_LAUNCH_W((k_search_solo_sets<MT, NCH, RT, 1, T>), a, T);
		if (c.regs <= 2)
			VSS_LAUNCH_W((k_search_solo_sets<MT, NCH, RT, 2, T>), a, T);
		if (c.regs <= 4)
			VSS_LAUNCH_W((k_search_solo_sets<MT, NCH, RT, 4, T>), a, T);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH_W((k_search_solo_sets<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
		VSS_LAUNCH_W((k_search_solo_sets<MT, NCH, RT, 0, T>), a, T);
	}
	if (a.gv.filter_bits & FILTER_BY_RANGE) {
		if (c.regs <= 1)
			VSS_LAUNCH_W((k_search_solo_ranges<MT, NCH, RT, 1, T>), a, T);
		if (c.regs <= 2)
			VSS_LAUNCH_W((k_search_solo_ranges<MT, NCH, RT, 2, T>), a, T);
		if (c.regs <= 4)
			VSS_LAUNCH_W((k_search_solo_ranges<MT, NCH, RT, 4, T>), a, T);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH_W((k_search_solo_ranges<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
		VSS_LAUNCH_W((k_search_solo_ranges<MT, NCH, RT, 0, T>), a, T);
	}
	if (a.gv.filter_bits & FILTER_BY_LABEL) {
		if (c.regs <= 1)
			VSS_LAUNCH_W((k_search_solo_labels<MT, NCH, RT, 1, T>), a, T);
		if (c.regs <= 2)
			VSS_LAUNCH_W((k_search_solo_labels<MT, NCH, RT, 2, T>), a, T);
		if (c.regs <= 4)
			VSS_LAUNCH_W((k_search_solo_labels<MT, NCH, RT, 4, T>), a, T);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH_W((k_search_solo_labels<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
		VSS_LAUNCH_W((k_search_solo_labels<MT, NCH, RT, 0, T>), a, T);
	}
	if (a.gv.filter_bits & FILTER_PER_QUERY) {
		if (c.regs <= 1)
			VSS_LAUNCH_W((k_search_solo_groups<MT, NCH, RT, 1, T>), a, T);
		if (c.regs <= 2)
			VSS_LAUNCH_W((k_search_solo_groups<MT, NCH, RT, 2, T>), a, T);
		if (c.regs <= 4)
			VSS_LAUNCH_W((k_search_solo_groups<MT, NCH, RT, 4, T>), a, T);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH_W((k_search_solo_groups<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
		VSS_LAUNCH_W((k_search_solo_groups<MT, NCH, RT, 0, T>), a, T);
	}
	if (c.regs <= 1)
		VSS_LAUNCH_W((k_search_solo<MT, NCH, RT, 1, T>), a, T);
	if (c.regs <= 2)
		VSS_LAUNCH_W((k_search_solo<MT, NCH, RT, 2, T>), a, T);
	if (c.regs <= 4)
		VSS_LAUNCH_W((k_search_solo<MT, NCH, RT, 4, T>), a, T);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_W((k_search_solo<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
	VSS_LAUNCH_W((k_search_solo<MT, NCH, RT, 0, T>), a, T);
}
template <int MT, int NCH, int R>
static hipError_t search_solo_e(const SearchArgs &a, const LaunchCfg &c) {
	if constexpr (NCH <= 1) {
		if (c.threads == 64 * VSS_TEAM_WAVES)
			return search_team_e<MT, NCH>(a, c);
	}
	constexpr int RS = NCH == 1 ? 16 : (NCH == 6 || NCH == 4) ? 4 : 8;
	if (a.gv.filter_bits & FILTER_BY_SET) {
		if (c.regs <= 1)
			VSS_LAUNCH((k_search_solo_sets<MT, NCH, RS, 1>), a);
		if (c.regs <= 2)
			VSS_LAUNCH((k_search_solo_sets<MT, NCH, RS, 2>), a);
		if (c.regs <= 4)
			VSS_LAUNCH((k_search_solo_sets<MT, NCH, RS, 4>), a);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH((k_search_solo_sets<MT, NCH, RS, MAX_LIST_REGS>), a);
		VSS_LAUNCH((k_search_solo_sets<MT, NCH, RS, 0>), a);
	}
	if (a.gv.filter_bits & FILTER_BY_RANGE) {
		if (c.regs <= 1)
			VSS_LAUNCH((k_search_solo_ranges<MT, NCH, RS, 1>), a);
		if (c.regs <= 2)
			VSS_LAUNCH((k_search_solo_ranges<MT, NCH, RS, 2>), a);
		if (c.regs <= 4)
			VSS_LAUNCH((k_search_solo_ranges<MT, NCH, RS, 4>), a);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH((k_search_solo_ranges<MT, NCH, RS, MAX_LIST_REGS>), a);
		VSS_LAUNCH((k_search_solo_ranges<MT, NCH, RS, 0>), a);
	}
	if (a.gv.filter_bits & FILTER_BY_LABEL) {
		if (c.regs <= 1)
			VSS_LAUNCH((k_search_solo_labels<MT, NCH, RS, 1>), a);
		if (c.regs <= 2)
			VSS_LAUNCH((k_search_solo_labels<MT, NCH, RS, 2>), a);
		if (c.regs <= 4)
			VSS_LAUNCH((k_search_solo_labels<MT, NCH, RS, 4>), a);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH((k_search_solo_labels<MT, NCH, RS, MAX_LIST_REGS>), a);
		VSS_LAUNCH((k_search_solo_labels<MT, NCH, RS, 0>), a);
	}
	if (a.gv.filter_bits & FILTER_PER_QUERY) {
		if (c.regs <= 1)
			VSS_LAUNCH((k_search_solo_groups<MT, NCH, RS, 1>), a);
		if (c.regs <= 2)
			VSS_LAUNCH((k_search_solo_groups<MT, NCH, RS, 2>), a);
		if (c.regs <= 4)
			VSS_LAUNCH((k_search_solo_groups<MT, NCH, RS, 4>), a);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH((k_search_solo_groups<MT, NCH, RS, MAX_LIST_REGS>), a);
		VSS_LAUNCH((k_search_solo_groups<MT, NCH, RS, 0>), a);
	}
	if (c.regs <= 1)
		VSS_LAUNCH((k_search_solo<MT, NCH, RS, 1>), a);
	if (c.regs <= 2)
		VSS_LAUNCH((k_search_solo<MT, NCH, RS, 2>), a);
	if (c.regs <= 4)
		VSS_LAUNCH((k_search_solo<MT, NCH, RS, 4>), a);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH((k_search_solo<MT, NCH, RS, MAX_LIST_REGS>), a);
	VSS_LAUNCH((k_search_solo<MT, NCH, RS, 0>), a);
}
template <int MT, int NCH, int R>
static hipError_t phase_a_e(const BuildArgs &a, const LaunchCfg &c) {
	if (c.regs <= 2)
		VSS_LAUNCH((k_build_phase_a<MT, NCH, R, 2>), a);
	if (c.regs <= 4)
		VSS_LAUNCH((k_build_phase_a<MT, NCH, R, 4>), a);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH((k_build_phase_a<MT, NCH, R, MAX_LIST_REGS>), a);
	VSS_LAUNCH((k_build_phase_a<MT, NCH, R, 0>), a);
}

// Phase A with 4 instead of 8 rows in flight per wave at dim 768: a third wave per SIMD, and refine_'s early exit works
// on passes of 4 kept neighbours instead of 8 (11 % fewer distances computed, same decisions): phase A -5.7 % at
// 3M x 768.  Phase B measured 5 % slower that way and keeps 8.
#define VSS_BY_CHUNKS_BUILD(FN, ...)                                                                                   \
	switch (c.nch) {                                                                                                   \
	case 1:                                                                                                            \
		return FN<VSS_MT, 1, 8>(__VA_ARGS__);                                                                          \
	case 2:                                                                                                            \
		return FN<VSS_MT, 2, 4>(__VA_ARGS__);                                                                          \
	case 3:                                                                                                            \
		return FN<VSS_MT, 3, VSS_BUILD_R3>(__VA_ARGS__);                                                               \
	case 4:                                                                                                            \
		return FN<VSS_MT, 4, 4>(__VA_ARGS__);                                                                          \
	case 6:                                                                                                            \
		return FN<VSS_MT, 6, 4>(__VA_ARGS__);                                                                          \
	default:                                                                                                           \
		return FN<VSS_MT, 0, 4>(__VA_ARGS__);                                                                          \
	}
#ifndef VSS_BUILD_R3
#define VSS_BUILD_R3 4
#endif

template <int MT, int NCH, int R>
static hipError_t phase_b_e(const LinkArgs &a, const LaunchCfg &c) {
	VSS_LAUNCH((k_build_phase_b<MT, NCH, R>), a);
}
template <int MT, int NCH, int R>
static hipError_t clusters_e(const ClusterArgs &a, const LaunchCfg &c) {
	VSS_LAUNCH((k_node_clusters<MT, NCH, R>), a);
}
template <int MT, int NCH, int R>
static hipError_t rerank_e(const RerankArgs &a, const LaunchCfg &c) {
	VSS_LAUNCH((k_exact_rerank<MT, NCH, R>), a);
}

template <>
hipError_t launch_search<VSS_MT>(const SearchArgs &a, const LaunchCfg &c) {
	if (filter_by_box(a.gv.filter_bits)) // (either box: before any of its bits alone; their walkers are units of their own)
		return launch_search_boxes<VSS_MT>(a, c);
	if (filter_by_set_box(a.gv.filter_bits)) // (after both boxes, before FILTER_BY_SET and FILTER_BY_LABEL, which are tested singly)
		return launch_search_set_boxes<VSS_MT>(a, c);
	VSS_BY_CHUNKS(search_e, a, c)
}
template <>
hipError_t launch_search_solo<VSS_MT>(const SearchArgs &a, const LaunchCfg &c) {
	if (filter_by_box(a.gv.filter_bits))
		return launch_search_solo_boxes<VSS_MT>(a, c);
	if (filter_by_set_box(a.gv.filter_bits))
		return launch_search_solo_set_boxes<VSS_MT>(a, c);
	VSS_BY_CHUNKS(search_solo_e, a, c)
}
template <>
hipError_t launch_phase_a<VSS_MT>(const BuildArgs &a, const LaunchCfg &c) {
	VSS_BY_CHUNKS_BUILD(phase_a_e, a, c)
}
#ifndef VSS_PHASE_B_R3
#define VSS_PHASE_B_R3 8 // rows in flight per pass of the link repair at 768 dimensions (A/B builds)
#endif
template <>
hipError_t launch_phase_b<VSS_MT>(const LinkArgs &a, const LaunchCfg &c) {
	if (c.nch == 3)
		return phase_b_e<VSS_MT, 3, VSS_PHASE_B_R3>(a, c);
	VSS_BY_CHUNKS(phase_b_e, a, c)
}
template <>
hipError_t launch_clusters<VSS_MT>(const ClusterArgs &a, const LaunchCfg &c) {
	VSS_BY_CHUNKS(clusters_e, a, c)
}
template <>
hipError_t launch_rerank<VSS_MT>(const RerankArgs &a, const LaunchCfg &c) {
	VSS_BY_CHUNKS(rerank_e, a, c)
}

} // namespace vss
