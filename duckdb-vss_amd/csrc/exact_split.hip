// exact_split.hip — the split-bf16 score tile of the exact search and its launchers (exact_split_kernels.h).  Built without
// packed f32 arithmetic (duckdb-vss_amd/__init__.py TU_FLAGS), hence a translation unit of its own.
#include <hip/hip_runtime.h>
#include <type_traits>

#define VSS_EXACT_SPLIT_TU
#include "exact_kernels.h"
