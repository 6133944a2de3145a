// exact_codes_probe <metric 0|1|2> <dim> <seed> — host check of the int8 bound tiles' UPPER bound (csrc/exact_codes_bound.h) over
// codes made with csrc/row_codes.h's own functions.  Per scale a line "scale pairs bad": `bad` = pairs whose U is below the
// float64 distance plus the engine's rounding term (none may be).  Then "slack pairs over": pairs of N(0, 1) rows whose U - d
// exceeds what range_codes_slack reports for the query; last "guards cases bad": records without a bound give +inf.
#include "../duckdb-vss_amd/csrc/exact_codes_bound.h"
#include "../duckdb-vss_amd/csrc/row_codes.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace vss;
typedef std::vector<float> Vec;

static RowCodeMeta encode(const Vec &v, std::vector<int> &codes) { // k_encode_rows' loop
	float amax = 0.f;
	bool finite = true;
	for (float x : v)
		finite = finite && fabsf(x) < INFINITY, amax = fmaxf(amax, fabsf(x));
	const float scale = finite ? row_code_scale(amax) : 0.f;
	double e2 = 0.0, n2 = 0.0;
	for (float x : v) {
		codes.push_back(scale > 0.f ? row_code_of(x, scale) : 0);
		const double r = scale > 0.f ? row_code_residual(x, scale, codes.back()) : 0.0;
		e2 += r * r, n2 += (double)x * (double)x;
	}
	return row_code_meta(scale, e2, n2, finite);
}

static double dot(const Vec &a, const Vec &b) {
	double s = 0;
	for (size_t i = 0; i < a.size(); ++i)
		s += (double)a[i] * b[i];
	return s;
}

static float upper(int metric, const Vec &q, const Vec &x, RowCodeMeta *mq_out = nullptr) {
	std::vector<int> cq, cx;
	const RowCodeMeta mq = encode(q, cq), mx = encode(x, cx);
	int I = 0;
	for (size_t i = 0; i < q.size(); ++i)
		I += cq[i] * cx[i];
	if (mq_out)
		*mq_out = mq;
	const uint32_t n = (uint32_t)q.size();
	return exact_codes_upper(I, exact_codes_query(metric, n, mq), exact_codes_row(metric, n, mx));
}

// the float64 distance, and what the engine's f32 value may exceed it by (exact_codes_bound.h's rounding terms)
static double distance(int metric, const Vec &q, const Vec &x, double &rounding) {
	const uint32_t n = (uint32_t)q.size();
	const double ab = dot(q, x), A = sqrt(dot(q, q)), B = sqrt(dot(x, x)), u = 0x1p-24, gn = exact_cert_gamma(n);
	if (metric == 2) {
		rounding = (gn + u * (1.0 + gn)) * A * B + u;
		return 1.0 - ab;
	}
	if (metric == 1) {
		rounding = range_codes_cos_engine(n);
		return 1.0 - ab / (A * B);
	}
	double l2 = 0;
	for (uint32_t i = 0; i < n; ++i)
		l2 += ((double)q[i] - x[i]) * ((double)q[i] - x[i]);
	rounding = exact_cert_gamma(n + 2.0) * (A + B) * (A + B);
	return l2;
}

int main(int argc, char **argv) {
	if (argc != 4)
		return 2;
	const int metric = atoi(argv[1]);
	const uint32_t n = (uint32_t)atoi(argv[2]);
	std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
	std::normal_distribution<float> g(0.f, 1.f);
	int over = 0;
	for (float scale : {1e-3f, 1.f, 1e3f}) {
		int bad = 0;
		for (int p = 0; p < 256; ++p) {
			Vec q(n), x(n);
			for (uint32_t i = 0; i < n; ++i)
				q[i] = scale * g(rng), x[i] = scale * g(rng);
			if (p & 1) // near-duplicates: the pairs a top-k is decided by
				for (uint32_t i = 0; i < n; ++i)
					x[i] = q[i] * (1.f + 1e-2f * x[i] / scale);
			double rounding;
			const double d = distance(metric, q, x, rounding);
			RowCodeMeta mq;
			const float U = upper(metric, q, x, &mq);
			bad += !((double)U >= d + rounding);
			if (scale == 1.f) // what the bound gives away, against the SLACK reported for a row of this norm
				over += !((double)U - d <= range_codes_slack(metric, n, mq, (float)dot(x, x)));
		}
		printf("%g 256 %d\n", scale, bad);
	}
	printf("slack 256 %d\n", over);
	int cases = 0, bad = 0; // no bound: zero, non-finite components, norms beyond the guards, on either side
	for (int c = 0; c < 8; ++c)
		for (int side = 0; side < 2; ++side, ++cases) {
			Vec q(n), x(n);
			for (uint32_t i = 0; i < n; ++i)
				q[i] = g(rng), x[i] = g(rng);
			Vec &v = side ? q : x;
			const float by[8] = {0.f, 1.f, 1.f, 1.f, 0x1p41f, 0x1p-45f, 0x1p60f, 0x1p-70f};
			for (uint32_t i = 0; i < n; ++i)
				v[i] *= by[c];
			if (c >= 1 && c <= 3)
				v[c * (n / 4)] = c == 1 ? INFINITY : c == 2 ? NAN : -INFINITY;
			bad += !(upper(metric, q, x) == INFINITY);
		}
	{ // a dimension beyond the model (n u >= 0.01 or n > 2^16), whatever the records say
		const RowCodeMeta m = {1.f / 127.f, 0.01f, 1.f, 0};
		for (uint32_t big : {65537u, 200000u}) {
			bad += !(exact_codes_upper(0, exact_codes_query(metric, big, m), exact_codes_row(metric, big, m)) == INFINITY);
			++cases;
		}
	}
	printf("guards %d %d\n", cases, bad);
	return 0;
}
