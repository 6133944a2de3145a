// exact_range.h — the score threshold of the exact RANGE search (vss_search_range_batch).
//
// A pure function of plain numbers — no HIP types — compiled for the device (k_range_prepare, exact_range_kernels.h) and, by
// tests/range_threshold_probe.cpp, for the host.
//
// Query q matches the live rows whose engine distance d (finish_distance, wave order) satisfies d <= r.  The candidate tile
// sees only a row's RANKING SCORE s (exact_certificate.h: g(s) is the distance s stands for, E bounds |d - g(s)| over all rows
// and every summation order).  A matching row has g(s) <= d + E <= r + E, and g is increasing, so with
//     theta = the smallest f32 that is not below g^-1(r + E)        l2sq  r + E - |q|^2    cosine  (r + E - 1) |q|    ip  r + E - 1
// no row with s > theta can match: the tile drops those and hands the rest — !(s > theta), which keeps a NaN score — to the
// re-score in the metric itself, which decides.  Where the model gives no finite E (norms outside 2^-40 .. 2^40, values that
// are not finite numbers) theta = +inf: every live row is re-scored.  A radius that can match nothing (NaN; negative under
// l2sq and cosine, whose distances the contract takes as non-negative) gets theta = -inf.
// The arithmetic here is float64; its own roundings — and those of g, which exact_cert_distance evaluates in float64 as well —
// are covered by a slack of 2^-45 (|r| + E + c), c = |q|^2 or 1: at least 2^20 units in the last place of every intermediate,
// and below 2^-21 E since E >= 2^-24 c.  The result is rounded UP to f32 and moved one more f32 up.
#pragma once
#include "exact_certificate.h"

namespace vss {

// one launch of the candidate tile covers at most RANGE_QUERY_BLOCK queries x RANGE_ROW_CHUNK rows: every pair of it fits the
// fixed candidate buffer of RANGE_QUERY_BLOCK * RANGE_ROW_CHUNK cells (8 bytes each: 64 MiB)
constexpr uint32_t RANGE_ROW_CHUNK = 8192, RANGE_QUERY_BLOCK = 1024;

// the next f32 above x (x finite or -inf; +inf and NaN stay)
VSS_CERT_HD inline float range_next_up(float x) {
	if (!(x < (float)INFINITY))
		return x;
	if (x == 0.f)
		return 0x1p-149f;
	union {
		float f;
		uint32_t u;
	} v;
	v.f = x;
	if (x == -(float)INFINITY)
		v.u = 0xFF7FFFFFu; // -FLT_MAX
	else
		v.u = x > 0.f ? v.u + 1u : v.u - 1u;
	return v.f;
}

// the smallest f32 that is not below t, one further up
VSS_CERT_HD inline float range_round_up(double t) {
	const double fmax = 0x1.fffffep127;
	if (!(t <= fmax))
		return t == t ? (float)INFINITY : (float)NAN;
	if (t < -fmax)
		return -(float)fmax;
	float f = (float)t;
	if ((double)f < t)
		f = range_next_up(f);
	return range_next_up(f);
}

// theta_q.  E = exact_cert_error of this query (computed once per query from the cached norm extrema)
VSS_CERT_HD inline float range_score_threshold(int metric, float radius, float qn2, double E) {
	if (!(E < (double)INFINITY))
		return (float)INFINITY; // no model: every live row is a candidate
	if (!(radius == radius) || (metric != 2 && radius < 0.f))
		return -(float)INFINITY; // matches nothing
	const double r = radius, c = metric == 0 ? (double)qn2 : 1.0;
	const double slack = 0x1p-45 * (fabs(r) + E + c);
	double t = r + E + slack - c;
	if (metric == 1) {
		t *= sqrt((double)qn2);
		t += fabs(t) * 0x1p-50;
	}
	return range_round_up(t);
}

// does distance d match radius r?  A plain f32 compare, but for the contract's special radii: NaN and (l2sq, cosine) negative
// radii match nothing, +inf matches the finite distances only.
VSS_CERT_HD inline bool range_matches(int metric, float d, float r) {
	if (metric != 2 && r < 0.f)
		return false;
	if (!(d <= r))
		return false;
	return r < (float)INFINITY || (d > -(float)INFINITY && d < (float)INFINITY);
}

} // namespace vss
