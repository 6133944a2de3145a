// exact_codes.hip — the exact search's int8 bound tile over the row codes, the kernels around it and their launchers
// (exact_codes_kernels.h).  A translation unit of its own, built without packed f32 arithmetic as exact_range_codes.hip is
// (duckdb-vss_amd/__init__.py TU_FLAGS): the bound's f32 operations are the ones exact_codes_bound.h counts.
#include <hip/hip_runtime.h>
#include <type_traits>

#define VSS_EXACT_CODES_TU
#include "exact_kernels.h"
