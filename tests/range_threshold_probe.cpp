// range_threshold_probe.cpp — stand-alone program behind tests/test_range_threshold_logic.py (plain g++, no HIP): the score
// threshold of the exact range search (duckdb-vss_amd/csrc/exact_range.h).
//   range_threshold_probe run <metric 0|1|2> <dim> <seed>
//       one line per case:  case queries matching_pairs violations inf_mismatches queries_without_E kept_share
//       matching_pairs = (query, radius, row) triples with float64 distance <= r, violations = those among them whose f32 score
//       exceeds theta with the dot product in one accumulator (the MFMA's order) or in wave order (must be 0), inf_mismatches =
//       (query, radius) pairs with (theta == +inf) != (E not finite) (must be 0), kept_share = triples theta keeps as candidates
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../duckdb-vss_amd/csrc/exact_range.h"

using namespace vss;

namespace {

float dot_sequential(const float *a, const float *b, size_t n) {
	float acc = 0.f;
	for (size_t i = 0; i != n; ++i)
		acc = std::fmaf(a[i], b[i], acc);
	return acc;
}
// wave order: lane g takes float4 chunks g, g + 64, ..., component by component, then the xor butterfly (32, 16, ..., 1)
float dot_wave(const float *a, const float *b, size_t n) {
	float lane[64];
	for (size_t g = 0; g != 64; ++g) {
		float acc = 0.f;
		for (size_t c = g; c < n / 4; c += 64)
			for (size_t k = 0; k != 4; ++k)
				acc = std::fmaf(a[4 * c + k], b[4 * c + k], acc);
		lane[g] = acc;
	}
	for (int off = 32; off; off >>= 1) {
		float next[64];
		for (int l = 0; l != 64; ++l)
			next[l] = lane[l] + lane[l ^ off];
		std::memcpy(lane, next, sizeof lane);
	}
	return lane[0];
}
// the score tiles' epilogue (exact_score, exact_kernels.h)
float score(int metric, float dot, float xn2) {
	if (metric == 0)
		return xn2 - 2.f * dot;
	if (metric == 2)
		return -dot;
	return xn2 > 0.f ? -dot * (1.0f / std::sqrt(xn2)) : 0.f;
}
double distance64(int metric, const float *q, const float *x, size_t n) {
	double ab = 0, a2 = 0, b2 = 0, l2 = 0;
	for (size_t i = 0; i != n; ++i) {
		const double a = q[i], b = x[i];
		ab += a * b, a2 += a * a, b2 += b * b, l2 += (a - b) * (a - b);
	}
	return metric == 0 ? l2 : metric == 2 ? 1.0 - ab : 1.0 - ab / std::sqrt(a2 * b2);
}

int run(int metric, size_t dim, uint64_t seed) {
	const size_t n = (dim + 3) / 4 * 4, rows = 1500, queries = 8;
	for (const char *name : {"random", "unit", "offset2048", "huge"}) {
		std::mt19937_64 rng(seed);
		std::normal_distribution<float> N(0.f, 1.f);
		std::vector<float> x(rows * n, 0.f), q(queries * n, 0.f), c(dim);
		for (auto &v : c)
			v = N(rng);
		double cs = 0;
		for (float v : c)
			cs += (double)v * v;
		const std::string s(name);
		const float offset = s == "offset2048" ? (float)(2048.0 / std::sqrt(cs)) : 0.f, scale = s == "huge" ? 0x1p41f : 1.f;
		auto fill = [&](std::vector<float> &v, size_t count) {
			for (size_t r = 0; r != count; ++r) {
				double ss = 0;
				for (size_t i = 0; i != dim; ++i) {
					v[r * n + i] = (c[i] * offset + N(rng)) * scale;
					ss += (double)v[r * n + i] * v[r * n + i];
				}
				for (size_t i = 0; s == "unit" && i != dim; ++i)
					v[r * n + i] = (float)(v[r * n + i] / std::sqrt(ss));
			}
		};
		fill(x, rows), fill(q, queries);
		std::vector<float> xn2(rows);
		float hi = 0.f, lo = INFINITY;
		for (size_t r = 0; r != rows; ++r) {
			xn2[r] = dot_wave(&x[r * n], &x[r * n], n);
			hi = std::fmax(hi, xn2[r]), lo = std::fmin(lo, xn2[r]);
		}
		size_t matching = 0, violations = 0, inf_mismatches = 0, without_E = 0, kept = 0, triples = 0;
		for (size_t qi = 0; qi != queries; ++qi) {
			const float *qv = &q[qi * n];
			const float qn2 = dot_wave(qv, qv, n);
			const double E = exact_cert_error(metric, (uint32_t)n, qn2, hi, lo);
			without_E += !(E < INFINITY);
			std::vector<double> d64(rows), sorted;
			std::vector<float> s0(rows), s1(rows);
			for (size_t r = 0; r != rows; ++r) {
				d64[r] = distance64(metric, qv, &x[r * n], n);
				s0[r] = score(metric, dot_sequential(qv, &x[r * n], n), xn2[r]);
				s1[r] = score(metric, dot_wave(qv, &x[r * n], n), xn2[r]);
			}
			sorted = d64;
			std::sort(sorted.begin(), sorted.end());
			// radii: at the nearest row, the 5th, the 100th, the median and beyond the farthest — rounded to f32 either way
			for (const double at : {sorted[0], sorted[4], sorted[99], sorted[rows / 2], sorted[rows - 1] * 1.5}) {
				for (const float r : {(float)at, std::nextafterf((float)at, -INFINITY), std::nextafterf((float)at, INFINITY)}) {
					const float theta = range_score_threshold(metric, r, qn2, E);
					inf_mismatches += (theta == INFINITY) != !(E < INFINITY);
					for (size_t row = 0; row != rows; ++row, ++triples) {
						kept += !(s0[row] > theta);
						if (d64[row] <= (double)r) {
							++matching;
							violations += s0[row] > theta || s1[row] > theta;
						}
					}
				}
			}
		}
		std::printf("%s %zu %zu %zu %zu %zu %.4f\n", name, queries, matching, violations, inf_mismatches, without_E, (double)kept / (double)triples);
	}
	return 0;
}

} // namespace

int main(int argc, char **argv) {
	if (argc == 5 && std::string(argv[1]) == "run")
		return run(std::atoi(argv[2]), (size_t)std::atoll(argv[3]), (uint64_t)std::atoll(argv[4]));
	std::fprintf(stderr, "usage: range_threshold_probe run <metric> <dim> <seed>\n");
	return 2;
}
