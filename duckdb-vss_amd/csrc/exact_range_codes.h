// exact_range_codes.h — the pair test of the exact RANGE search's int8 candidate tiles (option range.codes_i8, score kind 2;
// exact_range_codes_kernels.h): which (query, row) pairs the integer dot product of two 8-bit codes may drop.
//
// Pure functions of plain numbers — no HIP types — compiled for the device (k_range_prepare_codes and the tiles' epilogue) and, by
// tests/range_codes_probe.cpp, for the host.
//
// Rows and queries are coded alike (row_codes.h):  q = sq cq + eq,  x = sx cx + ex,  |eq|_2 <= errq,  |ex|_2 <= errx,  codes in
// -127 .. 127, and the tile computes  I = sum cq_i cx_i  EXACTLY (i32; n <= 2^16 keeps |I| < 2^31).  In real arithmetic
//     q.x = sq sx I + (sq cq).ex + eq.x,   |sq cq| = |q - eq| <= |q| + errq,   so
//     q.x <= U := sq sx I + (|q| + errq) errx + errq |x|.
// With A = |q|, B = |x| (real norms; the records' f32 `norm` is within 2^-23 of them, taken as Nq, Nx times 1 +- 2^-22), u = 2^-24,
// gamma(m) as in exact_certificate.h, the engine's f32 distance d (finish_distance, any summation order) has the lower bounds
//   * ip      d = fl(1 - dot):  d >= 1 - q.x - g A B - u,  g = gamma(n) + u (1 + gamma(n))           (the engine side of the ip E)
//   * l2sq    d = sum fl(q_i - x_i)^2 >= A^2 + B^2 - 2 q.x - gamma(n + 2) (A + B)^2,  (A + B)^2 <= 2 A^2 + 2 B^2
//   * cosine  d >= 1 - q.x / (A B) - Ec,  Ec = (gamma(n) + r + u) (1 + r) (1 + u)^2 + 2 u  (the engine side of the cosine E; it
//             needs both norms inside the guards below, which also keeps metric_cos_gt's zero-norm cases out)
// A pair is DROPPED only if such a bound, with U in the place of q.x, is above the radius.  Each of the three tests is brought
// into one form, so that the epilogue does a handful of f32 operations per pair:
//     W = sqm sx I + errx c1 + Nx c2 - m(x);      drop iff W < c3;      keep = !(W < c3)   (a NaN keeps the pair)
//   ip      sqm = sq     c1 = Nq+ + errq       c2 = errq + g Nq+                m = 0                       c3 = 1 - r - u
//   l2sq    sqm = 2 sq   c1 = 2 (Nq+ + errq)   c2 = 2 errq                      m = (1 - 2 gamma(n + 2)) Nx^2   c3 = Nq-^2 - 2 gamma(n + 2) Nq+^2 - r
//   cosine  sqm = sq     c1 = Nq+ + errq       c2 = errq - kappa Nq-/+          m = 0                       c3 = 0,  kappa = 1 - r - Ec
// (Nq+ / Nq-: the norm moved outward; under cosine kappa Nq Nx is rounded down whatever kappa's sign, and Nx's own 2^-22 goes
// into the constants of the query: c2 is multiplied by 1 + 2^-22 where it is positive, m carries 1 - 2^-20.)  The per-query
// constants {sqm, c1, c2, c3} are computed ONCE per query in float64 (range_codes_query) and rounded outward — c1, c2 up, c3
// down; the per-row values {sx, errx, Nx, m} come from the row's record (range_codes_row).
//
// Why the f32 evaluation of W (range_codes_keep: one convert, one multiply, three fma) cannot drop a pair the real inequality
// keeps: the terms are bounded by  |sqm sx I| <= c1 (Nx + errx)  (|sq cq| <= |q| + errq, |sx cx| <= |x| + errx, Cauchy-Schwarz),
// errx c1, Nx |c2| and m <= Nx^2; each is computed with at most three roundings and they are added by three fma, so the computed
// W is within 8 u (c1 (Nx + 2 errx) + Nx |c2| + Nx^2) of the real one.  range_codes_query adds 2^-19 c1 to c1 and
// 2^-19 (c1 + |c2|) to c2, range_codes_row takes 2^-19 off m's factor: an explicit outward slack of 2^-19 >= 4 x 8 u on every
// term, which also covers the roundings of the constants themselves.  Products below the normal range (errx may be tiny) add at
// most a few 2^-149, and c3 is moved down by 2^-120 and two f32 steps for them.
//
// ALWAYS kept (c3 = -inf, or the row's `free` flag): a query or row whose record says "no bound" (err = +inf, scale 0: a
// non-finite component, an all-zero vector), a norm outside 2^-39 .. 2^39 (inside exact_certificate.h's 2^-40 .. 2^40 guard by the
// norms' own rounding; cosine's zero-norm sides fall here), n u >= 0.01 or n > 2^16, a radius of +inf.  A radius that matches
// nothing (NaN; negative under l2sq and cosine) gets c3 = +inf: the metric would refuse every pair of it anyway.  The metric
// decides every kept pair afterwards, so special radii behave as with the other tiles.
//
// SLACK (vss_last_range_scores [2]): per query, the distance the bound gives away at a row of the largest live norm Bmax whose
// residual is the codes' nominal worst, errx = sqrt(n) / 254 Bmax (half a code step in every component):
//     ip  (Nq + errq) errx + errq Bmax + g Nq Bmax + u      l2sq  twice the first two terms + gamma(n + 2) (Nq + Bmax)^2
//     cosine  ((Nq + errq) errx + errq Bmax) / (Nq Bmax) + Ec
// the call reports the largest finite one over its queries, as a double's bit pattern.  A report, not part of any proof.
#pragma once
#include "exact_range.h"
#include "prescore_bound.h"

namespace vss {

struct RangeCodesQuery { // per query, 16 bytes: read as one float4 by the epilogue
	float sqm, c1, c2, c3;
};
struct RangeCodesRow { // per row, from its RowCodeMeta
	float sx, errx, nx, m;
	bool free; // no bound: every pair of this row is kept
};

VSS_CERT_HD inline float range_codes_up(double x) { // the smallest f32 >= x, one further up
	return range_round_up(x);
}
VSS_CERT_HD inline float range_codes_down(double x) { // the largest f32 <= x, two further down
	return -range_next_up(range_round_up(-x));
}
VSS_CERT_HD inline bool range_codes_norm_ok(double norm) {
	return norm >= 0x1p-39 && norm <= 0x1p39;
}
VSS_CERT_HD inline bool range_codes_meta_ok(const RowCodeMeta &m) {
	return m.err < (float)INFINITY && m.err >= 0.f && m.scale > 0.f && m.scale < (float)INFINITY && range_codes_norm_ok(m.norm);
}
VSS_CERT_HD inline double range_codes_cos_engine(uint32_t n) { // Ec
	const double u = 0x1p-24, gn = exact_cert_gamma(n);
	const double h = 1.0 / sqrt(1.0 - gn) - 1.0;
	const double rd = (1.0 + h) * (1.0 + h) * (1.0 + 2.0 * u) * (1.0 + 2.0 * u) * (1.0 + u) - 1.0, r = rd / (1.0 - rd);
	return ((gn + r + u) * (1.0 + r) * (1.0 + u) * (1.0 + u) + 2.0 * u) * (1.0 + 0x1p-20);
}

// the constants of query `qm` (its code record) under radius `radius`; n = the padded dimension
VSS_CERT_HD inline RangeCodesQuery range_codes_query(int metric, uint32_t n, float radius, const RowCodeMeta &qm) {
	const RangeCodesQuery keep_all = {0.f, 0.f, 0.f, -(float)INFINITY}, drop_all = {0.f, 0.f, 0.f, (float)INFINITY};
	if (!(radius == radius) || (metric != 2 && radius < 0.f))
		return drop_all;
	if (!range_codes_meta_ok(qm) || !((double)n * 0x1p-24 < 0.01) || n > 65536u || !(radius < (float)INFINITY))
		return keep_all;
	const double u = 0x1p-24, w = 0x1p-22, r = radius;
	const double nq_hi = (double)qm.norm * (1.0 + w), nq_lo = (double)qm.norm * (1.0 - w), errq = qm.err;
	const double gn = exact_cert_gamma(n), gn2 = exact_cert_gamma(n + 2.0);
	double sqm = qm.scale, c1 = nq_hi + errq, c2, c3;
	if (metric == 2) {
		c2 = errq + (gn + u * (1.0 + gn)) * nq_hi * (1.0 + 0x1p-20);
		c3 = 1.0 - r - u - 0x1p-50 * (1.0 + fabs(r));
	} else if (metric == 0) {
		sqm *= 2.0, c1 *= 2.0;
		c2 = 2.0 * errq;
		c3 = nq_lo * nq_lo * (1.0 - 0x1p-50) - 2.0 * gn2 * nq_hi * nq_hi * (1.0 + 0x1p-20) - r;
		c3 -= 0x1p-50 * (nq_hi * nq_hi + r);
	} else {
		const double kappa = 1.0 - r - range_codes_cos_engine(n) - 0x1p-50 * (2.0 + r); // (rounded down)
		// drop iff U < kappa A B: kappa A B is taken at its smallest, so both norms move down for kappa > 0 and up otherwise;
		// Nx's share of that is the 1 -+ 2^-21 here
		c2 = errq - (kappa > 0.0 ? kappa * nq_lo * (1.0 - 0x1p-21) : kappa * nq_hi * (1.0 + 0x1p-21));
		c3 = 0.0;
	}
	if (c2 > 0.0)
		c2 *= 1.0 + w; // Nx+ in the place of Nx
	const double c1s = c1 + 0x1p-19 * c1, c2s = c2 + 0x1p-19 * (c1 + fabs(c2));
	RangeCodesQuery o;
	o.sqm = (float)sqm; // (exact: a power of two times an f32)
	o.c1 = range_codes_up(c1s), o.c2 = range_codes_up(c2s), o.c3 = range_codes_down(c3 - 0x1p-120);
	if (!(o.sqm < (float)INFINITY) || !(o.c1 < (float)INFINITY) || !(o.c2 == o.c2) || !(o.c3 == o.c3))
		return keep_all;
	return o;
}

// the values of a row (its code record) the pair test reads
VSS_CERT_HD inline RangeCodesRow range_codes_row(int metric, uint32_t n, const RowCodeMeta &xm) {
	RangeCodesRow o;
	o.free = !range_codes_meta_ok(xm);
	o.sx = xm.scale, o.errx = xm.err, o.nx = xm.norm, o.m = 0.f;
	if (metric == 0) { // B-^2 - 2 gamma(n + 2) B+^2, less the evaluation's slack; float64, rounded down
		const double k = 1.0 - 0x1p-20 - 2.0 * exact_cert_gamma(n + 2.0) * (1.0 + 0x1p-20) - 0x1p-19;
		o.m = range_codes_down((double)xm.norm * (double)xm.norm * k);
		if (!(o.m >= 0.f))
			o.m = 0.f;
	}
	return o;
}

// the pair test: I = the integer dot product of the two codes.  true = the pair is proposed to the metric.
VSS_CERT_HD inline bool range_codes_keep(int I, const RangeCodesQuery &q, const RangeCodesRow &x) {
	const float w = fmaf((float)I, q.sqm * x.sx, fmaf(x.errx, q.c1, fmaf(x.nx, q.c2, -x.m)));
	return x.free || !(w < q.c3);
}

// SLACK of one query (see above); +inf where the query is always kept.  xn2_max: the largest f32 sum of squares over the live rows
VSS_CERT_HD inline double range_codes_slack(int metric, uint32_t n, const RowCodeMeta &qm, float xn2_max) {
	if (!range_codes_meta_ok(qm) || !(xn2_max >= 0.f) || !(xn2_max < (float)INFINITY) || !((double)n * 0x1p-24 < 0.01))
		return (double)INFINITY;
	const double u = 0x1p-24, gn = exact_cert_gamma(n), A = qm.norm, B = sqrt((double)xn2_max), errq = qm.err;
	const double errx = sqrt((double)n) / 254.0 * B, cross = (A + errq) * errx + errq * B;
	if (metric == 2)
		return cross + (gn + u * (1.0 + gn)) * A * B + u;
	if (metric == 0)
		return 2.0 * cross + exact_cert_gamma(n + 2.0) * (A + B) * (A + B);
	return B > 0.0 ? cross / (A * B) + range_codes_cos_engine(n) : (double)INFINITY;
}

} // namespace vss
