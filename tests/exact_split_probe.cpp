// exact_split_probe.cpp — stand-alone program behind tests/test_exact_split_bf16_logic.py: the two-way bf16 split
// (duckdb-vss_amd/csrc/split_bf16.h) and the error bound of the score built on it (exact_cert_error_split,
// duckdb-vss_amd/csrc/exact_certificate.h), checked in float64 on the host.  Plain g++, no HIP, no GPU.
//
//   exact_split_probe <metric 0|1|2> <dim> <seed>
//       per kind of data (random, offset, alternating):  kind pairs recon_bad split_bad total_bad cert_bad worst_split worst_total
//         recon_bad  elements with |x - hi| > 2^-8 |x| or |x - hi - lo| > 2^-16 |x|
//         split_bad  (query, row) pairs whose exact three-term sum is further than the header's split term from the exact q.x
//         total_bad  pairs whose three-term sum, accumulated in f32 in a shuffled order, is further than sigma A B + F from q.x
//         cert_bad   pairs with exact_cert_error_split < exact_cert_error;   worst_*: the largest error / bound seen
//       then  guards <cases> <bad>:  norms in and out of the model's range, inf, NaN — bad = the split form finite where the
//       f32 form is not, or the reverse, or smaller
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../duckdb-vss_amd/csrc/exact_certificate.h"
#include "../duckdb-vss_amd/csrc/split_bf16.h"

using namespace vss;

int main(int argc, char **argv) {
	if (argc != 4)
		return 2;
	const int metric = atoi(argv[1]);
	const size_t n = (size_t)atoi(argv[2]);
	std::mt19937_64 rng((uint64_t)atoll(argv[3]));
	std::normal_distribution<float> normal(0.f, 1.f);
	std::uniform_real_distribution<float> uni(0.f, 1.f);
	const size_t rows = 64, queries = 4;
	const char *kinds[3] = {"random", "offset", "alternating"};
	for (int kind = 0; kind != 3; ++kind) {
		// random: N(0, 1); offset: a common vector of norm 8192 plus N(0, 1); alternating: signs + - + -, magnitudes 2^-20 .. 2^20
		std::vector<float> common(n);
		double cn = 0;
		for (auto &v : common)
			v = normal(rng), cn += (double)v * v;
		for (auto &v : common)
			v = (float)(v * 8192.0 / std::sqrt(cn));
		auto make = [&](std::vector<float> &out, size_t count) {
			out.resize(count * n);
			for (size_t r = 0; r != count; ++r)
				for (size_t i = 0; i != n; ++i) {
					float v = normal(rng);
					if (kind == 1)
						v += common[i];
					if (kind == 2)
						v = ((i & 1) ? -1.f : 1.f) * std::ldexp(1.f + uni(rng), (int)(uni(rng) * 41.f) - 20);
					out[r * n + i] = v;
				}
		};
		std::vector<float> X, Q;
		make(X, rows);
		make(Q, queries);
		uint64_t recon_bad = 0, split_bad = 0, total_bad = 0, cert_bad = 0;
		double worst_split = 0, worst_total = 0;
		auto split_all = [&](const std::vector<float> &v, std::vector<float> &hi, std::vector<float> &lo) {
			hi.resize(v.size()), lo.resize(v.size());
			for (size_t i = 0; i != v.size(); ++i) {
				const SplitBf16 s = split_bf16(v[i]);
				hi[i] = bf16_value(s.hi), lo[i] = bf16_value(s.lo);
				const double x = v[i];
				if (std::fabs(x - hi[i]) > 0x1p-8 * std::fabs(x) || std::fabs(x - hi[i] - lo[i]) > 0x1p-16 * std::fabs(x))
					++recon_bad;
			}
		};
		std::vector<float> Xh, Xl, Qh, Ql;
		split_all(X, Xh, Xl);
		split_all(Q, Qh, Ql);
		float xn2_max = 0.f, xn2_min = std::numeric_limits<float>::infinity();
		std::vector<double> xnorm(rows);
		for (size_t r = 0; r != rows; ++r) {
			float s = 0.f;
			double d = 0;
			for (size_t i = 0; i != n; ++i)
				s = std::fmaf(X[r * n + i], X[r * n + i], s), d += (double)X[r * n + i] * X[r * n + i];
			xn2_max = std::max(xn2_max, s), xn2_min = std::min(xn2_min, s);
			xnorm[r] = std::sqrt(d);
		}
		std::vector<float> terms(3 * n);
		for (size_t q = 0; q != queries; ++q) {
			float qn2 = 0.f;
			double qd = 0;
			for (size_t i = 0; i != n; ++i)
				qn2 = std::fmaf(Q[q * n + i], Q[q * n + i], qn2), qd += (double)Q[q * n + i] * Q[q * n + i];
			const double A = std::sqrt(qd);
			if (exact_cert_error_split(metric, (uint32_t)n, qn2, xn2_max, xn2_min) < exact_cert_error(metric, (uint32_t)n, qn2, xn2_max, xn2_min))
				++cert_bad;
			for (size_t r = 0; r != rows; ++r) {
				const float *x = &X[r * n], *xh = &Xh[r * n], *xl = &Xl[r * n];
				const float *y = &Q[q * n], *yh = &Qh[q * n], *yl = &Ql[q * n];
				long double dot = 0, three = 0;
				for (size_t i = 0; i != n; ++i) {
					dot += (long double)y[i] * x[i];
					three += (long double)yh[i] * xh[i] + (long double)yh[i] * xl[i] + (long double)yl[i] * xh[i];
					terms[3 * i] = yh[i] * xh[i], terms[3 * i + 1] = yh[i] * xl[i], terms[3 * i + 2] = yl[i] * xh[i]; // (exact: 8 x 8 bits)
				}
				std::shuffle(terms.begin(), terms.end(), rng);
				float acc = 0.f;
				for (float t : terms)
					acc += t;
				const double AB = A * xnorm[r];
				const double split_bound = exact_cert_split_term() * AB;
				const double total_bound = exact_cert_split_sigma((uint32_t)n) * AB + exact_cert_split_flush((uint32_t)n, A, xnorm[r]);
				const double es = (double)fabsl(dot - three), et = (double)fabsl(dot - (long double)acc);
				split_bad += es > split_bound, total_bad += et > total_bound;
				worst_split = std::max(worst_split, es / split_bound), worst_total = std::max(worst_total, et / total_bound);
			}
		}
		printf("%s %zu %llu %llu %llu %llu %.6f %.6f\n", kinds[kind], rows * queries, (unsigned long long)recon_bad,
		       (unsigned long long)split_bad, (unsigned long long)total_bad, (unsigned long long)cert_bad, worst_split, worst_total);
	}
	// the guards: finite exactly where the f32 form is, never smaller
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const float norms[] = {0.f, 0x1p-90f, 0x1p-81f, 0x1p-80f, 0x1p-40f, 1.f, 768.f, 0x1p40f, 0x1p80f, 0x1p81f, 0x1p100f, inf, nan, -1.f};
	uint64_t cases = 0, bad = 0;
	for (float a2 : norms)
		for (float b2 : norms)
			for (float bmin : norms)
				for (uint32_t dim : {(uint32_t)n, 200000u}) {
					const double f = exact_cert_error(metric, dim, a2, b2, bmin), s = exact_cert_error_split(metric, dim, a2, b2, bmin);
					++cases;
					bad += (std::isinf(f) != std::isinf(s)) || std::isnan(s) || s < f;
				}
	printf("guards %llu %llu\n", (unsigned long long)cases, (unsigned long long)bad);
	return 0;
}
