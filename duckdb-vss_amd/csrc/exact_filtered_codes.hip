// exact_filtered_codes.hip — the filtered exact search's int8 bound tile over the row codes, gathered through the predicates'
// lists, and its launcher (exact_filtered_codes_kernels.h).  A translation unit of its own, built without packed f32 arithmetic
// as exact_codes.hip is (duckdb-vss_amd/__init__.py TU_FLAGS): the bound's f32 operations are the ones exact_codes_bound.h counts.
#include <hip/hip_runtime.h>
#include <type_traits>

#define VSS_EXACT_FILTERED_CODES_TU
#include "exact_filtered_codes_kernels.h"
