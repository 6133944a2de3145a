// range_codes_probe <metric 0|1|2> <dim> <seed> — host check of the int8 range tiles' pair test (csrc/exact_range_codes.h) over
// codes made with csrc/row_codes.h's own functions.  Per kind of data a line "kind pairs bad far_dropped": `bad` = pairs dropped at
// a radius not below the true float64 distance (none may be), `far_dropped` = pairs dropped at a radius well below it (the test
// is not vacuous).  Last line "guards cases bad": records without a bound keep every pair at the smallest radius.
#include "../duckdb-vss_amd/csrc/exact_range_codes.h"
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

static bool kept(int metric, const Vec &q, const Vec &x, float r) {
	std::vector<int> cq, cx;
	const RowCodeMeta mq = encode(q, cq), mx = encode(x, cx);
	int I = 0;
	for (size_t i = 0; i < q.size(); ++i)
		I += cq[i] * cx[i];
	const uint32_t n = (uint32_t)q.size();
	return range_codes_keep(I, range_codes_query(metric, n, r, mq), range_codes_row(metric, n, mx));
}

static float not_below(double d) {
	const float f = (float)d;
	return (double)f < d ? nextafterf(f, INFINITY) : f;
}

int main(int argc, char **argv) {
	if (argc != 4)
		return 2;
	const int metric = atoi(argv[1]);
	const uint32_t n = (uint32_t)atoi(argv[2]);
	std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
	std::normal_distribution<float> g(0.f, 1.f);
	auto sign = [&] { return (rng() & 1) ? 1.f : -1.f; };
	const char *kinds[] = {"random", "offset", "near", "halfstep", "limits"};
	for (int kind = 0; kind < 5; ++kind) {
		int bad = 0, far_dropped = 0;
		for (int p = 0; p < 256; ++p) {
			Vec q(n), x(n);
			for (uint32_t i = 0; i < n; ++i) {
				q[i] = g(rng), x[i] = g(rng);
				if (kind == 1) // a common offset of 2048 in every component
					q[i] += 2048.f, x[i] += 2048.f;
				if (kind == 2) // near-duplicates
					x[i] = q[i] * (1.f + 1e-4f * x[i]);
				if (kind == 3) // components at +-0.5 code steps (the scale is 1: the largest component is 127, below)
					q[i] = sign() * ((float)(rng() % 127) + 0.5f), x[i] = sign() * ((float)(rng() % 127) + 0.5f);
			}
			if (kind == 3)
				q[0] = x[1] = 127.f;
			if (kind == 4) { // norms just inside the guards of the bound, in all four combinations
				const float s = ((p & 1) ? 0x1p38f : 0x1p-38f) / (float)sqrt(dot(q, q)), t = ((p & 2) ? 0x1p38f : 0x1p-38f) / (float)sqrt(dot(x, x));
				for (uint32_t i = 0; i < n; ++i)
					q[i] *= s, x[i] *= t;
			}
			const double ab = dot(q, x), a2 = dot(q, q), b2 = dot(x, x);
			double l2 = 0;
			for (uint32_t i = 0; i < n; ++i)
				l2 += ((double)q[i] - x[i]) * ((double)q[i] - x[i]);
			const double d = metric == 0 ? l2 : metric == 2 ? 1.0 - ab : 1.0 - ab / sqrt(a2 * b2);
			for (double r : {d, d + fabs(d) * 1e-6, d + fabs(d) + 1.0}) // at the distance itself, a little and a lot above it
				bad += !kept(metric, q, x, not_below(r));
			// half the distance; half of |q| |x| below it (ip's distances scale with the norms); half of cosine's unit
			far_dropped += !kept(metric, q, x, (float)(metric == 0 ? 0.5 * d : metric == 2 ? d - 0.5 * sqrt(a2 * b2) : d - 0.5));
		}
		printf("%s 256 %d %d\n", kinds[kind], bad, far_dropped);
	}
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
			bad += !kept(metric, q, x, metric == 2 ? -0x1p100f : 0.f);
		}
	printf("guards %d %d\n", cases, bad);
	return 0;
}
