// prescore_bound.h — the lower bound of a row's distance that the search engine's scoring waves compute from the row's
// 8-bit code (row_codes.h) BEFORE they read its f32 components: a row whose bound is not below the radius of a full
// candidate list is rejected without the 4 x dim bytes of the row itself ("Pre-scoring", has the derivation).
//
// Pure functions of plain numbers — no HIP types — compiled for the device and, by tests/prescore_probe.cpp, for the host.
//
// What is bounded is the distance AS THE ENGINE'S f32 ARITHMETIC COMPUTES IT (finish_distance, wave_primitives.h), in any
// summation order: with u = 2^-24 and n terms, a dot product summed in f32 (fma or not, any order) is off by at most
// n u / (1 - n u) x |x|.|y| <= n u' |x| |y|.  All of it is gathered into one relative slack per metric,
//     SLACK(dim) = (dim + 64) x 2^-21            (4e-4 at 768 dimensions; the codes' own error E / |r| is ~8e-3)
// which covers, each with its worst case, the engine's sum, the sum over the codes, the two norms and the final
// division / subtraction; the bound's own arithmetic is float64 and rounds its result DOWN to f32.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSS_PRESCORE_HD __host__ __device__
#else
#define VSS_PRESCORE_HD
#endif

namespace vss {

// per-row record next to the code bytes (16 bytes, read as one float4)
struct RowCodeMeta {
	float scale; // component i of the row is scale x code_i + e_i
	float err;   // >= |e|_2 in real arithmetic (rounded up); +inf = this row has no bound and is never rejected
	float norm;  // |row|_2, within one f32 rounding
	uint32_t spare;
};

constexpr float PRESCORE_NO_BOUND = -INFINITY; // below every distance and every radius: rejects nothing

VSS_PRESCORE_HD inline double prescore_slack(uint32_t dim) {
	return ((double)dim + 64.0) * (1.0 / 2097152.0); // 2^-21
}

// the largest f32 that is <= x (x finite or -inf)
VSS_PRESCORE_HD inline float prescore_round_down(double x) {
	float f = (float)x;
	if ((double)f > x)
		f = nextafterf(f, -INFINITY);
	return f;
}

// metric: 0 l2sq, 1 cosine, 2 ip.
//   t      = sum q_i x code_i, accumulated in f32 in any order (cosine, ip)
//   s2     = sum (q_i - scale x code_i)^2, accumulated in f32 in any order (l2sq)
//   q_norm = |q|_2 from an f32 sum of squares in any order (the engine's own |q|^2 under a square root)
// Returns a value <= the engine's f32 distance between q and the row, or PRESCORE_NO_BOUND.
VSS_PRESCORE_HD inline float prescore_bound(int metric, float t, float s2, const RowCodeMeta &m, float q_norm, uint32_t dim) {
	const double scale = m.scale, E = m.err, rn = m.norm, qn = q_norm;
	// "no bound": a row without a code, a zero-norm side (cosine's special cases), anything that is not a finite number, and
	// norms outside 2^-40 .. 2^40, where sums of products of two components may leave the normal f32 range (the error model
	// above assumes they do not)
	if (!(E < (double)INFINITY) || !(scale > 0.0) || !(rn >= 0x1p-40 && rn <= 0x1p40) || !(E <= rn))
		return PRESCORE_NO_BOUND;
	if (metric != 0 && !(qn >= 0x1p-40 && qn <= 0x1p40)) // (l2sq does not use |q|: a query out of range shows in s2)
		return PRESCORE_NO_BOUND;
	const double slack = prescore_slack(dim);
	double lb;
	if (metric == 0) {
		if (!(s2 >= 0.f) || !(s2 < INFINITY))
			return PRESCORE_NO_BOUND;
		// |q - r| >= |q - s c| - E, and the f32 s2 is within (slack / 2) |q - s c| + 4 u |s c| of the real |q - s c|^2's root
		double root = sqrt((double)s2) * (1.0 - 0.5 * slack) - E - 0x1p-21 * (rn + E);
		if (root < 0.0)
			root = 0.0;
		lb = root * root * (1.0 - slack) - 0x1p-120; // the engine's sum of squares: relative error only (and underflow)
	} else {
		if (!(fabsf(t) < INFINITY))
			return PRESCORE_NO_BOUND;
		const double ub = scale * (double)t + qn * E; // q.r <= s (q.c) + |q| E
		const double qr = qn * rn;
		if (metric == 1)
			lb = 1.0 - ub / qr - slack;
		else
			lb = 1.0 - ub - slack * qr - 0x1p-22 * (1.0 + qr);
	}
	if (!(lb == lb))
		return PRESCORE_NO_BOUND;
	return prescore_round_down(lb);
}

} // namespace vss
