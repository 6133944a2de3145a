// kernels_boxes.inc — the walkers of the launches with one BOX per query (vss_search_batch_by_label_box, filter_bits carries
// FILTER_BY_RANGE and FILTER_BY_SET together) and with one box of 64-bit ends per query (vss_search_batch_by_label_box64: all three
// BY_ bits), for ONE metric (VSS_MT), and their launchers.  Included by kernels_boxes_{l2sq,cosine,ip}.hip: translation units of
// their own beside kernels_{l2sq,cosine,ip}.hip, so that a build of the library compiles the 420 instantiations on cores the three
// metric units leave idle.  kernels_metric.inc's launch_search / launch_search_solo hand every launch with filter_by_box() here.
#include "launchers.h"

namespace vss {

#include "launch_macros.inc"

// launches with one box per query (filter_bits carries FILTER_BY_RANGE and FILTER_BY_SET together): the *_boxes kernels, the
// same ladders
template <int MT, int NCH, int R>
static hipError_t search_boxes_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.list_lds)
		VSS_LAUNCH_T((k_search_boxes<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search_boxes<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search_boxes<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search_boxes<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search_boxes<MT, NCH, RS, 0>), a, c.threads);
}
// launches with one box of 64-bit ends per query (filter_bits carries FILTER_BY_LABEL, FILTER_BY_RANGE and FILTER_BY_SET, all
// three): the *_boxes64 kernels, the same ladders
template <int MT, int NCH, int R>
static hipError_t search_boxes64_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.list_lds)
		VSS_LAUNCH_T((k_search_boxes64<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search_boxes64<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search_boxes64<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search_boxes64<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search_boxes64<MT, NCH, RS, 0>), a, c.threads);
}
template <int MT, int NCH, int R>
static hipError_t search_any_box_e(const SearchArgs &a, const LaunchCfg &c) {
	if (filter_by_box64(a.gv.filter_bits)) // (all three bits: before the box, which is two of them)
		return search_boxes64_e<MT, NCH, R>(a, c);
	return search_boxes_e<MT, NCH, R>(a, c);
}
// the few-query shapes, as kernels_metric.inc's search_team_e / search_solo_e have them for the other families
template <int MT, int NCH>
static hipError_t search_team_boxes_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int T = VSS_TEAM_WAVES, RT = VSS_TEAM_R;
	if (filter_by_box64(a.gv.filter_bits)) { // (before the box)
		if (c.regs <= 1)
			VSS_LAUNCH_W((k_search_solo_boxes64<MT, NCH, RT, 1, T>), a, T);
		if (c.regs <= 2)
			VSS_LAUNCH_W((k_search_solo_boxes64<MT, NCH, RT, 2, T>), a, T);
		if (c.regs <= 4)
			VSS_LAUNCH_W((k_search_solo_boxes64<MT, NCH, RT, 4, T>), a, T);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH_W((k_search_solo_boxes64<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
		VSS_LAUNCH_W((k_search_solo_boxes64<MT, NCH, RT, 0, T>), a, T);
	}
	if (filter_by_box(a.gv.filter_bits)) {
		if (c.regs <= 1)
			VSS_LAUNCH_W((k_search_solo_boxes<MT, NCH, RT, 1, T>), a, T);
		if (c.regs <= 2)
			VSS_LAUNCH_W((k_search_solo_boxes<MT, NCH, RT, 2, T>), a, T);
		if (c.regs <= 4)
			VSS_LAUNCH_W((k_search_solo_boxes<MT, NCH, RT, 4, T>), a, T);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH_W((k_search_solo_boxes<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
		VSS_LAUNCH_W((k_search_solo_boxes<MT, NCH, RT, 0, T>), a, T);
	}
	return hipErrorInvalidValue; // (not reached: the caller saw filter_by_box())
}
template <int MT, int NCH, int R>
static hipError_t search_solo_boxes_e(const SearchArgs &a, const LaunchCfg &c) {
	if constexpr (NCH <= 1) {
		if (c.threads == 64 * VSS_TEAM_WAVES)
			return search_team_boxes_e<MT, NCH>(a, c);
	}
	constexpr int RS = NCH == 1 ? 16 : (NCH == 6 || NCH == 4) ? 4 : 8;
	if (filter_by_box64(a.gv.filter_bits)) { // (before the box)
		if (c.regs <= 1)
			VSS_LAUNCH((k_search_solo_boxes64<MT, NCH, RS, 1>), a);
		if (c.regs <= 2)
			VSS_LAUNCH((k_search_solo_boxes64<MT, NCH, RS, 2>), a);
		if (c.regs <= 4)
			VSS_LAUNCH((k_search_solo_boxes64<MT, NCH, RS, 4>), a);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH((k_search_solo_boxes64<MT, NCH, RS, MAX_LIST_REGS>), a);
		VSS_LAUNCH((k_search_solo_boxes64<MT, NCH, RS, 0>), a);
	}
	if (filter_by_box(a.gv.filter_bits)) {
		if (c.regs <= 1)
			VSS_LAUNCH((k_search_solo_boxes<MT, NCH, RS, 1>), a);
		if (c.regs <= 2)
			VSS_LAUNCH((k_search_solo_boxes<MT, NCH, RS, 2>), a);
		if (c.regs <= 4)
			VSS_LAUNCH((k_search_solo_boxes<MT, NCH, RS, 4>), a);
		if (c.regs <= MAX_LIST_REGS)
			VSS_LAUNCH((k_search_solo_boxes<MT, NCH, RS, MAX_LIST_REGS>), a);
		VSS_LAUNCH((k_search_solo_boxes<MT, NCH, RS, 0>), a);
	}
	return hipErrorInvalidValue; // (not reached)
}

template <>
hipError_t launch_search_boxes<VSS_MT>(const SearchArgs &a, const LaunchCfg &c) {
	VSS_BY_CHUNKS(search_any_box_e, a, c)
}
template <>
hipError_t launch_search_solo_boxes<VSS_MT>(const SearchArgs &a, const LaunchCfg &c) {
	VSS_BY_CHUNKS(search_solo_boxes_e, a, c)
}

} // namespace vss
