// exact_range_codes.hip — the range search's int8 candidate tiles over the row codes and their launchers
// (exact_range_codes_kernels.h).  A translation unit of its own, built without packed f32 arithmetic as exact_range.hip is
// (duckdb-vss_amd/__init__.py TU_FLAGS): the pair test's f32 operations are the ones exact_range_codes.h counts.
#include <hip/hip_runtime.h>
#include <type_traits>

#define VSS_EXACT_RANGE_CODES_TU
#include "exact_range_kernels.h"
