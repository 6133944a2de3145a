// launchers.h — host-side launch functions of the templated kernels.  The kernels are instantiated per index metric
// in three translation units (kernels_l2sq.hip / kernels_cosine.hip / kernels_ip.hip, all built from
// kernels_metric.inc) so they compile in parallel; the engine picks the instantiation at run time.  The walkers of the launches
// by label box (both boxes: filter_by_box()) are three more units, kernels_boxes_{l2sq,cosine,ip}.hip from kernels_boxes.inc:
// launch_search / launch_search_solo hand such a launch to launch_search_boxes / launch_search_solo_boxes.  The walkers of the
// launches by label set box (filter_by_set_box()) are three more again, kernels_setboxes_{l2sq,cosine,ip}.hip from
// kernels_setboxes.inc, behind launch_search_set_boxes / launch_search_solo_set_boxes.
#pragma once
#include "exact_kernels.h"
#include "hnsw_kernels.h"

namespace vss {

struct LaunchCfg {
	uint32_t nch;  // float4 chunks per lane: V <= nch * G  (1, 3, 6 have unrolled instantiations, others loop)
	uint32_t regs; // registers needed by the candidate list = ceil(limit / 64)
	uint32_t grid;
	uint32_t lds; // dynamic LDS bytes
	uint32_t threads; // search engine: threads per workgroup (64 x (walkers + scoring waves))
	hipStream_t stream;
};

template <int MT>
hipError_t launch_search(const SearchArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_search_solo(const SearchArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_search_boxes(const SearchArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_search_solo_boxes(const SearchArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_search_set_boxes(const SearchArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_search_solo_set_boxes(const SearchArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_phase_a(const BuildArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_phase_b(const LinkArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_clusters(const ClusterArgs &a, const LaunchCfg &c);
template <int MT>
hipError_t launch_rerank(const RerankArgs &a, const LaunchCfg &c);

#define VSS_DECLARE_METRIC(MT)                                                                                         \
	template <>                                                                                                        \
	hipError_t launch_search<MT>(const SearchArgs &, const LaunchCfg &);                                               \
	template <>                                                                                                        \
	hipError_t launch_search_solo<MT>(const SearchArgs &, const LaunchCfg &);                                          \
	template <>                                                                                                        \
	hipError_t launch_search_boxes<MT>(const SearchArgs &, const LaunchCfg &);                                         \
	template <>                                                                                                        \
	hipError_t launch_search_solo_boxes<MT>(const SearchArgs &, const LaunchCfg &);                                    \
	template <>                                                                                                        \
	hipError_t launch_search_set_boxes<MT>(const SearchArgs &, const LaunchCfg &);                                     \
	template <>                                                                                                        \
	hipError_t launch_search_solo_set_boxes<MT>(const SearchArgs &, const LaunchCfg &);                                \
	template <>                                                                                                        \
	hipError_t launch_phase_a<MT>(const BuildArgs &, const LaunchCfg &);                                               \
	template <>                                                                                                        \
	hipError_t launch_phase_b<MT>(const LinkArgs &, const LaunchCfg &);                                                \
	template <>                                                                                                        \
	hipError_t launch_clusters<MT>(const ClusterArgs &, const LaunchCfg &);                                            \
	template <>                                                                                                        \
	hipError_t launch_rerank<MT>(const RerankArgs &, const LaunchCfg &);
VSS_DECLARE_METRIC(0)
VSS_DECLARE_METRIC(1)
VSS_DECLARE_METRIC(2)

} // namespace vss
