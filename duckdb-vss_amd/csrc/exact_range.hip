// exact_range.hip — the kernels of the exact range search and their launchers (exact_range_kernels.h).  Built without packed
// f32 arithmetic (duckdb-vss_amd/__init__.py TU_FLAGS), hence a translation unit of its own.
#include <hip/hip_runtime.h>
#include <type_traits>

#define VSS_EXACT_RANGE_TU
#include "exact_range_kernels.h"
