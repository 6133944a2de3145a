// launch_macros.inc — what the translation units that instantiate the templated kernels share (kernels_metric.inc,
// kernels_boxes.inc): the launch macros, the rows in flight of the engine's and the teams' shapes, the switch over chunks per lane.
template <typename K>
static hipError_t allow_big_lds(K kernel) {
	// > 64 KiB of dynamic LDS must be requested explicitly; 160 KiB is the gfx950 per-CU total
	return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
	                           160 * 1024);
}

#define VSS_LAUNCH_W(KERNEL, ARGS, WAVES)                                                                                      \
	do {                                                                                                               \
		auto kern = KERNEL;                                                                                            \
		hipError_t e = allow_big_lds(kern);                                                                            \
		if (e != hipSuccess)                                                                                           \
			return e;                                                                                                  \
		hipLaunchKernelGGL(kern, dim3(c.grid), dim3(64 * (WAVES)), c.lds, c.stream, ARGS);                             \
		return hipGetLastError();                                                                                      \
	} while (0)

#define VSS_LAUNCH(KERNEL, ARGS) VSS_LAUNCH_W(KERNEL, ARGS, 1)

#define VSS_LAUNCH_T(KERNEL, ARGS, THREADS)                                                                            \
	do {                                                                                                               \
		auto kern = KERNEL;                                                                                            \
		hipError_t e = allow_big_lds(kern);                                                                            \
		if (e != hipSuccess)                                                                                           \
			return e;                                                                                                  \
		hipLaunchKernelGGL(kern, dim3(c.grid), dim3(THREADS), c.lds, c.stream, ARGS);                                  \
		return hipGetLastError();                                                                                      \
	} while (0)

#ifndef VSS_SEARCH_R6
#define VSS_SEARCH_R6 2 // 6 chunks per lane (dimension 1536): 4 rows in flight spill 72 bytes per lane beyond the 128 VGPRs
#endif
// (a level-0 list of 32 rows at 128 dims: 4 rows per wave; A/B builds)
#ifndef VSS_TEAM_R
#define VSS_TEAM_R (VSS_TEAM_WAVES <= 4 ? 4 : 2)
#endif

// chunks per lane with unrolled instantiations: 1 (dimensions 4 .. 256 that fill a power-of-two group), 2 (512), 3 (768),
// 4 (1024), 6 (1536); every other dimension takes the looping variant (0)
#define VSS_BY_CHUNKS(FN, ...)                                                                                         \
	switch (c.nch) {                                                                                                   \
	case 1:                                                                                                            \
		return FN<VSS_MT, 1, 8>(__VA_ARGS__);                                                                          \
	case 2:                                                                                                            \
		return FN<VSS_MT, 2, 8>(__VA_ARGS__);                                                                          \
	case 3:                                                                                                            \
		return FN<VSS_MT, 3, 8>(__VA_ARGS__);                                                                          \
	case 4:                                                                                                            \
		return FN<VSS_MT, 4, 4>(__VA_ARGS__);                                                                          \
	case 6:                                                                                                            \
		return FN<VSS_MT, 6, 4>(__VA_ARGS__);                                                                          \
	default:                                                                                                           \
		return FN<VSS_MT, 0, 4>(__VA_ARGS__);                                                                          \
	}

