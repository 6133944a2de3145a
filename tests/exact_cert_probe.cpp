// exact_cert_probe.cpp — stand-alone program behind tests/test_exact_certificate_logic.py: the certificate of the exact search
// (duckdb-vss_amd/csrc/exact_certificate.h) checked on the host against a model of the engine's two sides — the metric in wave
// order (finish_distance) and the ranking score with its dot product in three summation orders (sequential fma like the
// MFMA's accumulator, pairwise over rounded products, wave order).
// Plain g++ (-ffp-contract=off), no HIP, no GPU; may also be built with -fsanitize=address,undefined.
//
//   exact_cert_probe run <metric 0|1|2> <dim> <k> <seed>
//       one line per case and order:  case order queries certified lost wrong bound_violations worst_ratio
//       certified = queries the certificate vouches for, lost = queries whose top-K' by score misses a row of the metric's
//       top-k, wrong = certified AND lost (must be 0), bound_violations = (query, row) pairs with |d - g(s)| > E (must be 0),
//       worst_ratio = the largest |d - g(s)| / E seen
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../duckdb-vss_amd/csrc/exact_certificate.h"

using namespace vss;

namespace {

// ---- f32 dot products in three orders
float dot_sequential(const float *a, const float *b, size_t n) {
	float acc = 0.f;
	for (size_t i = 0; i != n; ++i)
		acc = std::fmaf(a[i], b[i], acc);
	return acc;
}
float dot_pairwise(const float *a, const float *b, size_t lo, size_t hi) {
	if (hi - lo == 1)
		return a[lo] * b[lo];
	const size_t mid = lo + (hi - lo) / 2;
	return dot_pairwise(a, b, lo, mid) + dot_pairwise(a, b, mid, hi);
}
// wave order: lane g takes float4 chunks g, g + 64, ..., component by component, then the xor butterfly (32, 16, ..., 1);
// sub = true: terms (a_i - b_i)^2 instead of a_i b_i
float sum_wave(const float *a, const float *b, size_t n, bool sub) {
	float lane[64];
	const size_t chunks = n / 4;
	for (size_t g = 0; g != 64; ++g) {
		float acc = 0.f;
		for (size_t c = g; c < chunks; c += 64)
			for (size_t k = 0; k != 4; ++k) {
				const size_t i = 4 * c + k;
				if (sub) {
					const float t = a[i] - b[i];
					acc = std::fmaf(t, t, acc);
				} else
					acc = std::fmaf(a[i], b[i], acc);
			}
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
float dot_in(int order, const float *a, const float *b, size_t n) {
	return order == 0 ? dot_sequential(a, b, n) : order == 1 ? dot_pairwise(a, b, 0, n) : sum_wave(a, b, n, false);
}

// finish_distance (wave_primitives.h) over wave-order sums
float engine_distance(int metric, const float *q, const float *x, size_t n) {
	if (metric == 0)
		return sum_wave(q, x, n, true);
	const float ab = sum_wave(q, x, n, false);
	if (metric == 2)
		return 1.0f - ab;
	const float a2 = sum_wave(q, q, n, false), b2 = sum_wave(x, x, n, false);
	if (a2 == 0.f && b2 == 0.f)
		return 0.f;
	if (a2 == 0.f || b2 == 0.f)
		return 1.f;
	return 1.0f - ab / (std::sqrt(a2) * std::sqrt(b2));
}

// the score tiles' epilogue (exact_score, exact_kernels.h)
float score(int metric, float dot, float xn2) {
	if (metric == 0)
		return xn2 - 2.f * dot;
	if (metric == 2)
		return -dot;
	return xn2 > 0.f ? -dot * (1.0f / std::sqrt(xn2)) : 0.f;
}

struct Data {
	size_t rows, queries, n; // n = padded dimension
	std::vector<float> x, q;
};

Data make(const std::string &name, size_t dim, uint64_t seed) {
	std::mt19937_64 rng(seed);
	std::normal_distribution<float> N(0.f, 1.f);
	Data d;
	d.n = (dim + 3) / 4 * 4;
	d.rows = 1500, d.queries = 8;
	auto fill = [&](std::vector<float> &v, size_t count, auto gen) {
		v.assign(count * d.n, 0.f);
		for (size_t r = 0; r != count; ++r)
			for (size_t i = 0; i != dim; ++i)
				v[r * d.n + i] = gen(r, i);
	};
	auto normalize = [&](float *v) {
		double s = 0;
		for (size_t i = 0; i != dim; ++i)
			s += (double)v[i] * v[i];
		for (size_t i = 0; i != dim; ++i)
			v[i] = (float)(v[i] / std::sqrt(s));
	};
	if (name == "random") {
		fill(d.x, d.rows, [&](size_t, size_t) { return N(rng); });
		fill(d.q, d.queries, [&](size_t, size_t) { return N(rng); });
	} else if (name == "unit") {
		fill(d.x, d.rows, [&](size_t, size_t) { return N(rng); });
		fill(d.q, d.queries, [&](size_t, size_t) { return N(rng); });
		for (size_t r = 0; r != d.rows; ++r)
			normalize(&d.x[r * d.n]);
		for (size_t r = 0; r != d.queries; ++r)
			normalize(&d.q[r * d.n]);
	} else if (name == "offset2048" || name == "offset8192") {
		std::vector<float> c(dim);
		for (auto &v : c)
			v = N(rng);
		normalize(c.data());
		const float len = name == "offset2048" ? 2048.f : 8192.f;
		fill(d.x, d.rows, [&](size_t, size_t i) { return c[i] * len + N(rng); });
		fill(d.q, d.queries, [&](size_t, size_t i) { return c[i] * len + N(rng); });
	} else if (name == "scaled") { // rows of very different lengths
		fill(d.x, d.rows, [&](size_t r, size_t) { return N(rng) * (r % 3 == 0 ? 1000.f : r % 3 == 1 ? 1.f : 0.001f); });
		fill(d.q, d.queries, [&](size_t r, size_t) { return N(rng) * (r % 2 ? 30.f : 0.03f); });
	} else if (name == "dominant") { // one component a thousand times the others
		fill(d.x, d.rows, [&](size_t, size_t i) { return N(rng) * (i == 1 ? 1000.f : 1.f); });
		fill(d.q, d.queries, [&](size_t, size_t i) { return N(rng) * (i == 1 ? 1000.f : 1.f); });
	} else if (name == "near_duplicates") { // 4 groups of 60 rows = unit vector + 1e-4 N(0, 1) among unit rows; queries inside the groups
		fill(d.x, d.rows, [&](size_t, size_t) { return N(rng); });
		for (size_t r = 0; r != d.rows; ++r)
			normalize(&d.x[r * d.n]);
		fill(d.q, d.queries, [&](size_t, size_t) { return 0.f; });
		for (size_t g = 0; g != 4; ++g) {
			std::vector<float> base(dim);
			for (auto &v : base)
				v = N(rng);
			normalize(base.data());
			for (size_t j = 0; j != 60; ++j) {
				const size_t r = (g * 60 + j) * 6 + 1; // scattered over the slots
				for (size_t i = 0; i != dim; ++i)
					d.x[r * d.n + i] = base[i] + 1e-4f * N(rng);
			}
			for (size_t j = 0; j != 2; ++j)
				for (size_t i = 0; i != dim; ++i)
					d.q[(2 * g + j) * d.n + i] = base[i] + 1e-4f * N(rng);
		}
	} else {
		std::fprintf(stderr, "unknown case %s\n", name.c_str());
		std::exit(2);
	}
	return d;
}

int run(int metric, size_t dim, size_t k, uint64_t seed) {
	const size_t KP = k + 8;
	for (const char *name : {"random", "unit", "offset2048", "offset8192", "scaled", "dominant", "near_duplicates"}) {
		const Data d = make(name, dim, seed);
		std::vector<float> xn2(d.rows);
		float hi = 0.f, lo = INFINITY;
		for (size_t r = 0; r != d.rows; ++r) {
			xn2[r] = sum_wave(&d.x[r * d.n], &d.x[r * d.n], d.n, false);
			hi = std::fmax(hi, xn2[r]), lo = std::fmin(lo, xn2[r]);
		}
		for (int order = 0; order != 3; ++order) {
			size_t certified = 0, lost = 0, wrong = 0, bound_violations = 0;
			double worst = 0.0;
			for (size_t qi = 0; qi != d.queries; ++qi) {
				const float *q = &d.q[qi * d.n];
				const float qn2 = sum_wave(q, q, d.n, false);
				const double E = exact_cert_error(metric, (uint32_t)d.n, qn2, hi, lo);
				std::vector<float> dist(d.rows), sc(d.rows);
				std::vector<uint32_t> by_score(d.rows), by_dist(d.rows);
				for (size_t r = 0; r != d.rows; ++r) {
					const float *x = &d.x[r * d.n];
					dist[r] = engine_distance(metric, q, x, d.n);
					sc[r] = score(metric, dot_in(order, q, x, d.n), xn2[r]);
					by_score[r] = by_dist[r] = (uint32_t)r;
					if (E < INFINITY) {
						const double off = std::fabs((double)dist[r] - exact_cert_distance(metric, sc[r], qn2));
						bound_violations += off > E;
						worst = std::fmax(worst, off / E);
					}
				}
				auto less_by = [](const std::vector<float> &v) {
					return [&v](uint32_t a, uint32_t b) { return v[a] < v[b] || (v[a] == v[b] && a < b); };
				};
				std::sort(by_score.begin(), by_score.end(), less_by(sc));
				std::sort(by_dist.begin(), by_dist.end(), less_by(dist));
				const size_t kept = std::min(KP, d.rows);
				bool is_lost = false;
				for (size_t j = 0; j != std::min(k, d.rows); ++j)
					is_lost = is_lost || std::find(by_score.begin(), by_score.begin() + kept, by_dist[j]) == by_score.begin() + kept;
				// the decision of k_exact_rerank
				const double floor_d = exact_cert_floor(metric, (uint32_t)d.n, sc[by_score[kept - 1]], qn2, hi, lo);
				size_t below = 0;
				for (size_t j = 0; j != kept; ++j)
					below += (double)dist[by_score[j]] < floor_d;
				const bool ok = E < INFINITY && (d.rows < KP || below >= k);
				certified += ok, lost += is_lost, wrong += ok && is_lost;
			}
			std::printf("%s %d %zu %zu %zu %zu %zu %.4f\n", name, order, d.queries, certified, lost, wrong, bound_violations, worst);
		}
	}
	return 0;
}

} // namespace

int main(int argc, char **argv) {
	if (argc == 6 && std::string(argv[1]) == "run")
		return run(std::atoi(argv[2]), (size_t)std::atoll(argv[3]), (size_t)std::atoll(argv[4]), (uint64_t)std::atoll(argv[5]));
	std::fprintf(stderr, "usage: exact_cert_probe run <metric> <dim> <k> <seed>\n");
	return 2;
}
