// exact_codes_bound.h — the UPPER bound of the exact top-k's int8 bound tiles (option exact.codes_i8, score kind 2;
// exact_codes_kernels.h): what the integer dot product of two 8-bit codes says a pair's distance cannot exceed.
// The mirror image of exact_range_codes.h, whose pair test is the LOWER bound of the same quantities.
//
// Pure functions of plain numbers — no HIP types — compiled for the device (k_exact_prepare_codes and the tile's epilogue) and,
// by tests/exact_codes_probe.cpp, for the host.
//
// With exact_range_codes.h's notation (q = sq cq + eq, x = sx cx + ex, |eq|_2 <= errq, |ex|_2 <= errx, I = sum cq_i cx_i exactly,
// A = |q|, B = |x|, the records' norms Nq, Nx within 1 +- w of them, w = 2^-22, u = 2^-24):
//     q.x = sq sx I + (sq cq).ex + eq.x,   |sq cq| <= A + errq,   so
//     q.x >= Lo := sq sx I - (A + errq) errx - errq B.
// The engine's f32 distance d (finish_distance, any summation order) has the upper bounds — the engine-side rounding terms of
// exact_range_codes.h, taken on the other side —
//   * ip      d = fl(1 - dot) <= 1 - q.x + g A B + u,   g = gamma(n) + u (1 + gamma(n))
//   * l2sq    d = sum fl(q_i - x_i)^2 <= A^2 + B^2 - 2 q.x + gamma(n + 2) (A + B)^2,   (A + B)^2 <= 2 A^2 + 2 B^2
//   * cosine  d <= 1 - q.x / (A B) + Ec,   Ec = range_codes_cos_engine(n)   (both norms inside the guards below)
// and with Lo in the place of q.x each becomes a bound U >= d from the codes alone.  All three are brought into ONE form,
//     T = -sqm sx I + errx c1 + Nx c2 + m(x),      U = rx T + c3
//   ip      sqm = sq        c1 = Nq+ + errq           c2 = errq + g Nq+     m = 0                      rx = 1       c3 = 1 + u
//   l2sq    sqm = 2 sq      c1 = 2 (Nq+ + errq)       c2 = 2 errq           m = (1 + 2 gamma(n+2)) Nx+^2   rx = 1       c3 = (1 + 2 gamma(n+2)) Nq+^2
//   cosine  sqm = sq / Nq-  c1 = (Nq+ + errq) / Nq-   c2 = errq / Nq-       m = 0                      rx = 1 / Nx-  c3 = 1 + Ec
// (Nq+ / Nq-: the record's norm times 1 +- w; c2 is multiplied by 1 + w for Nx+.)  Under cosine the positive part
// (A + errq) errx + errq B is divided by the smallest A B; the signed part -sq sx I / (A B) is taken at Nq- Nx-, which is within
// 1.3 x 2^-20 |sq sx I| / (A B) of its value at the real norms, and |sqm sx I| <= c1 (Nx+ + errx) by Cauchy-Schwarz.  The per-query
// constants {sqm, c1, c2, c3} are computed ONCE per query in float64 (exact_codes_query) and rounded up; the per-row values
// {sx, errx, Nx, m, rx} come from the row's record (exact_codes_row).
//
// Why the f32 evaluation (exact_codes_upper: one convert, one multiply, four fma) cannot fall below the real U: the terms are
// bounded by |sqm sx I| <= c1 (Nx+ + errx), errx c1, Nx c2, m and c3, each is computed with at most three roundings and they are
// added by four fma, so the computed value is within 8 u (= 2^-21) of the sum of their magnitudes (times rx) of the real one;
// under cosine the rounding of sqm adds 2^-24, rx's three f32 steps upward (they LOWER a negative T) 2^-21.4, and the norms
// 1.3 x 2^-20 of the signed term.  exact_codes_query adds 2^-18 c1 to c1, 2^-18 (c1 + c2) to c2 and 2^-18 c3 to c3,
// exact_codes_row 2^-18 to m's factor: an explicit upward slack of 2^-18 on every term — four times 2^-20, where less than
// two and a quarter are needed — which also covers the roundings of the constants themselves.
// Products below the normal range add at most a few 2^-149 (times rx <= 2^40): c3 is moved up by 2^-100 and two f32 steps.
//
// NO BOUND (U = +inf; such a pair never lowers a query's k-th smallest bound): the cases of range_codes_meta_ok — a record that
// says "no bound" (err = +inf, scale 0: a non-finite component, an all-zero vector) on either side, a norm outside
// 2^-39 .. 2^39 (cosine's zero norms fall here) —, n u >= 0.01 or n > 2^16, and an evaluation that is not a number.
#pragma once
#include "exact_range_codes.h"

namespace vss {

struct ExactCodesQuery { // per query, 16 bytes: read as one float4 by the epilogue
	float sqm, c1, c2, c3;
};
struct ExactCodesRow { // per row, from its RowCodeMeta
	float sx, errx, nx, m, rx;
	bool none; // no bound: U = +inf
};

// the constants of query `qm` (its code record); n = the padded dimension
VSS_CERT_HD inline ExactCodesQuery exact_codes_query(int metric, uint32_t n, const RowCodeMeta &qm) {
	const ExactCodesQuery none = {0.f, 0.f, 0.f, (float)INFINITY};
	if (!range_codes_meta_ok(qm) || !((double)n * 0x1p-24 < 0.01) || n > 65536u)
		return none;
	const double u = 0x1p-24, w = 0x1p-22, s = 0x1p-18;
	const double nq_hi = (double)qm.norm * (1.0 + w), nq_lo = (double)qm.norm * (1.0 - w), errq = qm.err;
	const double gn = exact_cert_gamma(n), gn2 = exact_cert_gamma(n + 2.0);
	double sqm = qm.scale, c1 = nq_hi + errq, c2, c3;
	if (metric == 2) {
		c2 = errq + (gn + u * (1.0 + gn)) * nq_hi * (1.0 + 0x1p-20);
		c3 = 1.0 + u;
	} else if (metric == 0) {
		sqm *= 2.0, c1 *= 2.0;
		c2 = 2.0 * errq;
		c3 = (1.0 + 2.0 * gn2 * (1.0 + 0x1p-20)) * nq_hi * nq_hi;
	} else {
		const double rq = (1.0 / nq_lo) * (1.0 + 0x1p-50);
		sqm *= rq, c1 *= rq;
		c2 = errq * rq;
		c3 = 1.0 + range_codes_cos_engine(n);
	}
	c2 *= 1.0 + w; // Nx+ in the place of Nx
	ExactCodesQuery o;
	o.sqm = (float)sqm; // (exact but under cosine, whose rounding the slack covers)
	o.c1 = range_codes_up(c1 + s * c1), o.c2 = range_codes_up(c2 + s * (c1 + c2)), o.c3 = range_codes_up(c3 + s * c3 + 0x1p-100);
	if (!(o.sqm < (float)INFINITY) || !(o.c1 < (float)INFINITY) || !(o.c2 < (float)INFINITY) || !(o.c3 < (float)INFINITY))
		return none;
	return o;
}

// the values of a row (its code record) the bound reads
VSS_CERT_HD inline ExactCodesRow exact_codes_row(int metric, uint32_t n, const RowCodeMeta &xm) {
	ExactCodesRow o;
	o.none = !range_codes_meta_ok(xm);
	o.sx = xm.scale, o.errx = xm.err, o.nx = xm.norm, o.m = 0.f, o.rx = 1.f;
	if (o.none)
		return o;
	if (metric == 0) { // (1 + 2 gamma(n + 2)) Nx+^2, plus the evaluation's slack; float64, rounded up
		const double k = (1.0 + 0x1p-20) * (1.0 + 2.0 * exact_cert_gamma(n + 2.0) * (1.0 + 0x1p-20)) + 0x1p-18;
		o.m = range_codes_up((double)xm.norm * (double)xm.norm * k);
	} else if (metric == 1)
		o.rx = range_codes_up(1.0 / ((double)xm.norm * (1.0 - 0x1p-22)) * (1.0 + 0x1p-50));
	return o;
}

// U: no engine distance of the pair is above it.  I = the integer dot product of the two codes.
VSS_CERT_HD inline float exact_codes_upper(int I, const ExactCodesQuery &q, const ExactCodesRow &x) {
	const float t = fmaf(-(float)I, q.sqm * x.sx, fmaf(x.errx, q.c1, fmaf(x.nx, q.c2, x.m)));
	const float U = fmaf(t, x.rx, q.c3);
	return (x.none || !(U == U)) ? (float)INFINITY : U;
}

} // namespace vss
