// exact_certificate.h — the per-query proof that the exact search's selection by RANKING SCORE kept the true top-k of the
// engine's own metric (DESIGN.md §4.4 has the derivation).
//
// Pure functions of plain numbers — no HIP types — compiled for the device (k_exact_rerank) and, by
// tests/exact_cert_probe.cpp, for the host.
//
// The exact path ranks every live row r by an f32 score s_r from the MFMA tile (|x|^2 - 2 q.x, -q.x / |x|, -q.x), keeps the
// K' smallest (score, slot) pairs S, and only re-scores S with the wave-order metric d_r (finish_distance,
// wave_primitives.h).  When the select passes end, every live row outside S has s_r >= tau_s, the largest score in S.  With
//     g(s)  the distance a score stands for:      l2sq  s + |q|^2      cosine  1 + s / |q|      ip  1 + s
//     E     a bound of |d_r - g(s_r)| over ALL rows r (both sides as the f32 arithmetic computes them, any summation order)
// g is increasing, so every row outside S has d_r >= g(s_r) - E >= g(tau_s) - E =: FLOOR.  If k members of S have d < FLOOR,
// the k smallest (d, slot) pairs of S are the k smallest of all live rows: the query is CERTIFIED.  Otherwise the engine
// redoes that query by brute force in the metric itself (k_exact_metric_scores).
//
// E, with u = 2^-24, gamma(m) = m u / (1 - m u), n = the padded dimension, A = |q|, B = max |x| (real norms, bounded from
// the f32 sums of squares a2, b2 by A^2 <= a2 / (1 - gamma(n))):
//   * a dot product or sum of squares of n terms accumulated in f32 — fused or not, in ANY order (the MFMA's, the
//     wave's, numpy's) — is within gamma(n + 1) |x| |y| of the real one: each product is rounded at most once and then
//     passes through at most n additions (Higham, Accuracy and Stability of Numerical Algorithms, §3.1);
//   * l2sq: d = sum fl(q_i - x_i)^2 is within gamma(n + 2) (A + B)^2 of |q - x|^2; the score xn2 - 2 dot is within
//     gamma(n + 1) (B^2 + 2 A B) of the real one, its own subtraction adds u (1 + gamma) (B^2 + 2 A B), |q|^2 adds
//     gamma(n) A^2:
//         E = (gamma(n + 2) + gamma(n + 1) + u (1 + gamma(n + 1))) (A + B)^2
//   * ip: d = fl(1 - dot_wave), g(s) = 1 - dot_mfma:
//         E = (gamma(n) + gamma(n + 1)) A B + u (1 + (1 + gamma(n)) A B)
//   * cosine: both sides are 1 - cos up to RELATIVE errors of the two norms' roots (h = (1 - gamma(n))^-1/2 - 1 each), the
//     roundings of sqrt, rsqrt (<= 4 u), multiply and divide, plus the dot product's gamma and the last subtraction's 2 u:
//         E = [engine] (gamma(n) + r + u) (1 + r) (1 + u)^2 + 2 u   +   [score] rs + gamma(n + 1) (1 + rs)
//         r = rd / (1 - rd), rd = (1 + h)^2 (1 + 2 u)^2 (1 + u) - 1;      rs = (1 + 4 u) (1 + h)^2 (1 + u) - 1
//     (|cos| <= 1 is all that is used of the rows, so no row norm enters — only the guard below).
// The model assumes that no sum leaves the normal f32 range: norms outside 2^-40 .. 2^40 (cosine: the smallest row norm as
// well, which also keeps metric_cos_gt's zero-norm special cases out) and anything that is not a finite number get NO
// certificate.  The certificate's own arithmetic is float64 and E is inflated by 2^-20 relative + 2^-100 for it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VSS_CERT_HD __host__ __device__
#else
#define VSS_CERT_HD
#endif

namespace vss {

VSS_CERT_HD inline double exact_cert_gamma(double m) {
	const double u = 0x1p-24;
	return m * u / (1.0 - m * u);
}

// g: the distance that score s stands for; qn2 = the query's f32 sum of squares (any order)
VSS_CERT_HD inline double exact_cert_distance(int metric, float s, float qn2) {
	if (metric == 0)
		return (double)s + (double)qn2;
	if (metric == 2)
		return 1.0 + (double)s;
	return 1.0 + (double)s / sqrt((double)qn2);
}

// E, or +inf where the model does not hold (no certificate).  n = padded dimension; xn2_max / xn2_min = the largest and
// smallest f32 sum of squares over the live rows.
VSS_CERT_HD inline double exact_cert_error(int metric, uint32_t n, float qn2, float xn2_max, float xn2_min) {
	const double u = 0x1p-24, lo = 0x1p-80, hi = 0x1p80; // squared norms of 2^-40 .. 2^40
	const double a2 = qn2, b2 = xn2_max, b2min = xn2_min;
	if (!(a2 >= 0.0 && a2 <= hi) || !(b2 >= 0.0 && b2 <= hi) || !((double)n * u < 0.01))
		return (double)INFINITY;
	if (metric == 1 && (!(a2 >= lo) || !(b2min >= lo)))
		return (double)INFINITY;
	const double gn = exact_cert_gamma(n), gn1 = exact_cert_gamma(n + 1.0), gn2 = exact_cert_gamma(n + 2.0);
	const double A = sqrt(a2 / (1.0 - gn)), B = sqrt(b2 / (1.0 - gn));
	double E;
	if (metric == 0)
		E = (gn2 + gn1 + u * (1.0 + gn1)) * (A + B) * (A + B);
	else if (metric == 2)
		E = (gn + gn1) * A * B + u * (1.0 + (1.0 + gn) * A * B);
	else {
		const double h = 1.0 / sqrt(1.0 - gn) - 1.0;
		const double rd = (1.0 + h) * (1.0 + h) * (1.0 + 2.0 * u) * (1.0 + 2.0 * u) * (1.0 + u) - 1.0, r = rd / (1.0 - rd);
		const double rs = (1.0 + 4.0 * u) * (1.0 + h) * (1.0 + h) * (1.0 + u) - 1.0;
		E = (gn + r + u) * (1.0 + r) * (1.0 + u) * (1.0 + u) + 2.0 * u + rs + gn1 * (1.0 + rs);
	}
	return E * (1.0 + 0x1p-20) + 0x1p-100;
}

// FLOOR: no live row outside the kept set has an engine distance below it (-inf = no certificate).  tau_s = the largest
// score of the (full) kept set, E = exact_cert_error of this query.
VSS_CERT_HD inline double exact_cert_floor_given(int metric, float tau_s, float qn2, double E) {
	const double g = exact_cert_distance(metric, tau_s, qn2);
	if (!(E < (double)INFINITY) || !(g > -(double)INFINITY && g < (double)INFINITY))
		return -(double)INFINITY;
	return g - E;
}
VSS_CERT_HD inline double exact_cert_floor(int metric, uint32_t n, float tau_s, float qn2, float xn2_max, float xn2_min) {
	return exact_cert_floor_given(metric, tau_s, qn2, exact_cert_error(metric, n, qn2, xn2_max, xn2_min));
}

} // namespace vss
