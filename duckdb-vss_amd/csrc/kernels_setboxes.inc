// kernels_setboxes.inc — the walkers of the launches with one IN-LIST on one label column inside a box of ranges per query
// (vss_search_batch_by_label_set_box: filter_bits carries FILTER_BY_LABEL and FILTER_BY_SET without FILTER_BY_RANGE), for ONE metric
// (VSS_MT), and their launchers.  Included by kernels_setboxes_{l2sq,cosine,ip}.hip: translation units of their own beside
// kernels_boxes_{l2sq,cosine,ip}.hip, so that a build of the library compiles them on cores the other units leave idle.
// kernels_metric.inc's launch_search / launch_search_solo hand every launch with filter_by_set_box() here.
#include "launchers.h"

namespace vss {

#include "launch_macros.inc"

// the *_set_boxes kernels, on the ladders of the *_boxes64 kernels
template <int MT, int NCH, int R>
static hipError_t search_set_boxes_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int RS = NCH == 6 ? VSS_SEARCH_R6 : 4;
	if (a.list_lds)
		VSS_LAUNCH_T((k_search_set_boxes<MT, NCH, RS, LDS_LIST_E>), a, c.threads);
	if (c.regs <= 2)
		VSS_LAUNCH_T((k_search_set_boxes<MT, NCH, RS, 2>), a, c.threads);
	if (c.regs <= 4)
		VSS_LAUNCH_T((k_search_set_boxes<MT, NCH, RS, 4>), a, c.threads);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_T((k_search_set_boxes<MT, NCH, RS, MAX_LIST_REGS>), a, c.threads);
	VSS_LAUNCH_T((k_search_set_boxes<MT, NCH, RS, 0>), a, c.threads);
}
// the few-query shapes, as kernels_boxes.inc has them for the boxes
template <int MT, int NCH>
static hipError_t search_team_set_boxes_e(const SearchArgs &a, const LaunchCfg &c) {
	constexpr int T = VSS_TEAM_WAVES, RT = VSS_TEAM_R;
	if (c.regs <= 1)
		VSS_LAUNCH_W((k_search_solo_set_boxes<MT, NCH, RT, 1, T>), a, T);
	if (c.regs <= 2)
		VSS_LAUNCH_W((k_search_solo_set_boxes<MT, NCH, RT, 2, T>), a, T);
	if (c.regs <= 4)
		VSS_LAUNCH_W((k_search_solo_set_boxes<MT, NCH, RT, 4, T>), a, T);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH_W((k_search_solo_set_boxes<MT, NCH, RT, MAX_LIST_REGS, T>), a, T);
	VSS_LAUNCH_W((k_search_solo_set_boxes<MT, NCH, RT, 0, T>), a, T);
}
template <int MT, int NCH, int R>
static hipError_t search_solo_set_boxes_e(const SearchArgs &a, const LaunchCfg &c) {
	if constexpr (NCH <= 1) {
		if (c.threads == 64 * VSS_TEAM_WAVES)
			return search_team_set_boxes_e<MT, NCH>(a, c);
	}
	constexpr int RS = NCH == 1 ? 16 : (NCH == 6 || NCH == 4) ? 4 : 8;
	if (c.regs <= 1)
		VSS_LAUNCH((k_search_solo_set_boxes<MT, NCH, RS, 1>), a);
	if (c.regs <= 2)
		VSS_LAUNCH((k_search_solo_set_boxes<MT, NCH, RS, 2>), a);
	if (c.regs <= 4)
		VSS_LAUNCH((k_search_solo_set_boxes<MT, NCH, RS, 4>), a);
	if (c.regs <= MAX_LIST_REGS)
		VSS_LAUNCH((k_search_solo_set_boxes<MT, NCH, RS, MAX_LIST_REGS>), a);
	VSS_LAUNCH((k_search_solo_set_boxes<MT, NCH, RS, 0>), a);
}

template <>
hipError_t launch_search_set_boxes<VSS_MT>(const SearchArgs &a, const LaunchCfg &c) {
	VSS_BY_CHUNKS(search_set_boxes_e, a, c)
}
template <>
hipError_t launch_search_solo_set_boxes<VSS_MT>(const SearchArgs &a, const LaunchCfg &c) {
	VSS_BY_CHUNKS(search_solo_set_boxes_e, a, c)
}

} // namespace vss
