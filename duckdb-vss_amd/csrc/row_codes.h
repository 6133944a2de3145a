// row_codes.h — 8-bit codes of the index's rows: derived data of the f32 vectors, read by the search engine's scoring waves
// ahead of the rows themselves (prescore_bound.h, DESIGN.md §4.2, "Pre-scoring").
//
// Per row (slot), two parts:
//   * V x 4 code bytes, one signed byte per float of the zero-padded row, in the row's own order: byte i codes component i,
//     so the dword at index c holds the four codes of float4 chunk c and lane g reads chunk g + ch x G of the codes exactly
//     where it reads chunk g + ch x G of the staged query (wave_distances' lane-to-dimension mapping);
//   * one 16-byte RowCodeMeta {scale, err, norm, spare}:  component_i = scale x code_i + e_i,  err >= |e|_2,  norm ~ |row|_2.
// scale = max |component| / 127 (f32), code_i = round(component_i / scale) clamped to -127 .. 127.  err and norm are
// accumulated in FLOAT64 — the residual component - scale x code is exact there (24 + 8 significant bits), a sum of n squares is
// off by n x 2^-53 relative — then err is multiplied by 1 + 2^-20 and rounded UP to f32: an upper bound in real arithmetic.
// A row with a non-finite component, or whose scale would be zero or denormal, gets err = +inf: "no bound", never rejected.
//
// The pure parts are host code as well (tests/prescore_probe.cpp restates the encoder's loop with them).
#pragma once
#include "prescore_bound.h"

#include <algorithm>

namespace vss {

// scale of a row whose largest finite |component| is amax; 0 = the row gets no code
VSS_PRESCORE_HD inline float row_code_scale(float amax) {
	const float scale = amax / 127.0f;
	return (scale >= 1.17549435e-38f && scale < INFINITY) ? scale : 0.f; // (FLT_MIN: zero and denormal scales are refused)
}
VSS_PRESCORE_HD inline int row_code_of(float x, float scale) {
	float c = rintf(x / scale);
	c = c > 127.f ? 127.f : c;
	c = c < -127.f ? -127.f : c;
	return (int)c;
}
// the residual of one component, exact in float64
VSS_PRESCORE_HD inline double row_code_residual(float x, float scale, int code) {
	return (double)x - (double)scale * (double)code;
}
// the record of a row from its float64 sums: e2 = sum of squared residuals, n2 = sum of squared components
VSS_PRESCORE_HD inline RowCodeMeta row_code_meta(float scale, double e2, double n2, bool finite) {
	RowCodeMeta m;
	m.scale = scale, m.spare = 0;
	m.norm = (float)sqrt(n2);
	if (!finite || !(scale > 0.f) || !(e2 == e2)) {
		m.scale = 0.f, m.err = INFINITY;
		return m;
	}
	const double e = sqrt(e2) * (1.0 + 0x1p-20);
	float f = (float)e;
	if ((double)f < e)
		f = nextafterf(f, INFINITY);
	m.err = f;
	return m;
}
VSS_PRESCORE_HD inline RowCodeMeta row_code_none() {
	return row_code_meta(0.f, 0.0, 0.0, false);
}

// ---------------------------------------------------------------------------------------------------------
// Which slots' codes are stale: ONE half-open range (the hull of everything marked since the last encode).  Every path
// that writes rows marks its slots — or everything —, and the index encodes the range before a search reads codes.
struct StaleSlots {
	uint64_t lo = 0, hi = 0; // empty when lo >= hi
	bool any() const {
		return lo < hi;
	}
	void mark(uint64_t first, uint64_t end) {
		if (first >= end)
			return;
		if (!any())
			lo = first, hi = end;
		else
			lo = std::min(lo, first), hi = std::max(hi, end);
	}
	void mark_all() {
		lo = 0, hi = ~0ull;
	}
	void clear() {
		lo = hi = 0;
	}
	// the slots to encode now, given that only slots below `rows` hold rows (the rest is encoded when rows get there: a slot
	// at or beyond `rows` that was marked stays marked)
	bool take(uint64_t rows, uint64_t &first, uint64_t &end) {
		first = lo, end = std::min(hi, rows);
		const bool work = first < end;
		if (hi <= rows)
			clear();
		else if (work)
			lo = rows;
		return work;
	}
};

#if defined(__HIPCC__)
// One wavefront per row, a grid-stride loop over slots [first, end).  Two passes over the row (the second one hits L2):
// the largest |component|, then codes, residuals and norm.  Plain vector stores, no atomics.
__global__ __launch_bounds__(256) void k_encode_rows(const float4 *vectors, uint32_t V, uint64_t first, uint64_t end, uint32_t *codes,
                                                     RowCodeMeta *meta) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
	for (uint64_t slot = first + (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); slot < end; slot += waves) {
		const float4 *row = vectors + slot * V;
		float amax = 0.f;
		bool finite = true;
		for (uint32_t c = lane; c < V; c += 64) {
			const float4 x = row[c];
			const float a = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w))); // (fmaxf drops a NaN: `finite` keeps it)
			finite = finite && fabsf(x.x) < INFINITY && fabsf(x.y) < INFINITY && fabsf(x.z) < INFINITY && fabsf(x.w) < INFINITY;
			amax = fmaxf(amax, a);
		}
		for (int off = 32; off; off >>= 1)
			amax = fmaxf(amax, __shfl_xor(amax, off));
		finite = __all(finite);
		const float scale = finite ? row_code_scale(amax) : 0.f;
		double e2 = 0.0, n2 = 0.0;
		for (uint32_t c = lane; c < V; c += 64) {
			const float4 x = row[c];
			const float xs[4] = {x.x, x.y, x.z, x.w};
			uint32_t word = 0;
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const int code = scale > 0.f ? row_code_of(xs[k], scale) : 0;
				const double r = scale > 0.f ? row_code_residual(xs[k], scale, code) : 0.0;
				e2 += r * r;
				n2 += (double)xs[k] * (double)xs[k];
				word |= ((uint32_t)code & 0xFFu) << (8 * k);
			}
			codes[slot * V + c] = word;
		}
		for (int off = 32; off; off >>= 1) {
			e2 += __shfl_xor(e2, off);
			n2 += __shfl_xor(n2, off);
		}
		if (lane == 0)
			meta[slot] = row_code_meta(scale, e2, n2, finite);
	}
}
#endif

} // namespace vss
