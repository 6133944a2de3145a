// prescore_probe.cpp — stand-alone program behind tests/test_prescore_logic.py: the pre-scoring bound
// (duckdb-vss_amd/csrc/prescore_bound.h) and the row encoder's arithmetic (duckdb-vss_amd/csrc/row_codes.h, whose kernel's
// loop is restated here on the host) checked against the engine's f32 distance computed in three summation orders.
// Plain g++ (-ffp-contract=off), no HIP, no GPU; may also be built with -fsanitize=address,undefined.
//
//   prescore_probe bound <metric 0|1|2> <dim> <pairs> <seed>    one line per case:  case pairs violations bounded worst_margin
//   prescore_probe degenerate <metric> <dim>                     one line per input: name bounded(0/1)
//   prescore_probe residual <dim> <rows> <seed>                  rows  violations  (stored err >= float64 residual norm)
//   prescore_probe stale <rounds> <seed>                         rounds violations (StaleSlots against a bitmap)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../duckdb-vss_amd/csrc/row_codes.h"

using namespace vss;

namespace {

struct Encoded {
	std::vector<int8_t> code;
	RowCodeMeta meta;
};

// k_encode_rows, one row, on the host (the order of the float64 sums differs: they are exact to 2^-53 either way)
Encoded encode(const std::vector<float> &row) {
	Encoded e;
	e.code.assign(row.size(), 0);
	float amax = 0.f;
	bool finite = true;
	for (float x : row) {
		finite = finite && std::fabs(x) < INFINITY;
		amax = std::fmax(amax, std::fabs(x));
	}
	const float scale = finite ? row_code_scale(amax) : 0.f;
	double e2 = 0.0, n2 = 0.0;
	for (size_t i = 0; i != row.size(); ++i) {
		const int c = scale > 0.f ? row_code_of(row[i], scale) : 0;
		const double r = scale > 0.f ? row_code_residual(row[i], scale, c) : 0.0;
		e2 += r * r;
		n2 += (double)row[i] * (double)row[i];
		e.code[i] = (int8_t)c;
	}
	e.meta = row_code_meta(scale, e2, n2, finite);
	return e;
}

// ---- f32 sums in three orders.  term(i, acc) adds term i to acc the way the engine's accumulate4 does (fma);
//      product(i) is the rounded term alone (the pairwise order adds rounded products)
template <class Term, class Product>
float sum_sequential(size_t n, Term term, Product) {
	float acc = 0.f;
	for (size_t i = 0; i != n; ++i)
		acc = term(i, acc);
	return acc;
}
template <class Product>
float pairwise(size_t lo, size_t hi, Product product) {
	if (hi - lo == 1)
		return product(lo);
	const size_t mid = lo + (hi - lo) / 2;
	return pairwise(lo, mid, product) + pairwise(mid, hi, product);
}
template <class Term, class Product>
float sum_pairwise(size_t n, Term, Product product) {
	return pairwise(0, n, product);
}
// wave order: lane g takes float4 chunks g, g + 64, ..., component by component, then the xor butterfly (32, 16, ..., 1)
template <class Term, class Product>
float sum_wave(size_t n, Term term, Product) {
	float lane[64];
	const size_t chunks = n / 4;
	for (size_t g = 0; g != 64; ++g) {
		float acc = 0.f;
		for (size_t c = g; c < chunks; c += 64)
			for (size_t k = 0; k != 4; ++k)
				acc = term(4 * c + k, acc);
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
template <class Term, class Product>
float sum_in(int order, size_t n, Term term, Product product) {
	return order == 0 ? sum_sequential(n, term, product) : order == 1 ? sum_pairwise(n, term, product) : sum_wave(n, term, product);
}

// finish_distance (wave_primitives.h)
float finish(int metric, float ab, float a2, float b2) {
	if (metric == 0)
		return ab;
	if (metric == 2)
		return 1.0f - ab;
	if (a2 == 0.f && b2 == 0.f)
		return 0.f;
	if (a2 == 0.f || b2 == 0.f)
		return 1.f;
	return 1.0f - ab / (std::sqrt(a2) * std::sqrt(b2));
}

float engine_distance(int metric, int order, const std::vector<float> &q, const std::vector<float> &x) {
	const size_t n = q.size();
	float ab, a2 = 0.f, b2 = 0.f;
	if (metric == 0) {
		ab = sum_in(order, n, [&](size_t i, float acc) { const float t = q[i] - x[i]; return std::fmaf(t, t, acc); },
		            [&](size_t i) { const float t = q[i] - x[i]; return t * t; });
	} else {
		ab = sum_in(order, n, [&](size_t i, float acc) { return std::fmaf(q[i], x[i], acc); }, [&](size_t i) { return q[i] * x[i]; });
	}
	if (metric == 1) {
		a2 = sum_in(order, n, [&](size_t i, float acc) { return std::fmaf(q[i], q[i], acc); }, [&](size_t i) { return q[i] * q[i]; });
		b2 = sum_in(order, n, [&](size_t i, float acc) { return std::fmaf(x[i], x[i], acc); }, [&](size_t i) { return x[i] * x[i]; });
	}
	return finish(metric, ab, a2, b2);
}

float bound_in(int metric, int order, const std::vector<float> &q, const Encoded &e, uint32_t dim) {
	const size_t n = q.size();
	const float s = e.meta.scale;
	float t = 0.f, s2 = 0.f;
	if (metric == 0) {
		s2 = sum_in(order, n,
		            [&](size_t i, float acc) { const float v = std::fmaf(-s, (float)e.code[i], q[i]); return std::fmaf(v, v, acc); },
		            [&](size_t i) { const float v = q[i] - s * (float)e.code[i]; return v * v; });
	} else {
		t = sum_in(order, n, [&](size_t i, float acc) { return std::fmaf(q[i], (float)e.code[i], acc); },
		           [&](size_t i) { return q[i] * (float)e.code[i]; });
	}
	const float a2 = sum_in(order, n, [&](size_t i, float acc) { return std::fmaf(q[i], q[i], acc); }, [&](size_t i) { return q[i] * q[i]; });
	return prescore_bound(metric, t, s2, e.meta, std::sqrt(a2), dim);
}

struct Tally {
	uint64_t pairs = 0, violations = 0, bounded = 0;
	double worst = INFINITY; // smallest (distance - bound) / scale seen among bounded pairs
};

void check_pair(int metric, uint32_t dim, const std::vector<float> &q, const std::vector<float> &x, Tally &t) {
	const Encoded e = encode(x);
	float d[3], b[3];
	for (int o = 0; o != 3; ++o)
		d[o] = engine_distance(metric, o, q, x), b[o] = bound_in(metric, o, q, e, dim);
	t.pairs++;
	bool bounded = true;
	for (int ob = 0; ob != 3; ++ob) {
		bounded = bounded && b[ob] > -INFINITY;
		for (int od = 0; od != 3; ++od) {
			// the property: bound <= distance; a distance that is NaN allows no bound at all
			const bool ok = d[od] != d[od] ? b[ob] == -INFINITY : !(b[ob] > d[od]);
			t.violations += !ok;
			if (b[ob] > -INFINITY && d[od] == d[od]) {
				const double unit = metric == 1 ? 1.0 : std::fmax(1e-30, std::fabs((double)d[od]) + (metric == 2 ? 1.0 : 0.0));
				t.worst = std::fmin(t.worst, ((double)d[od] - (double)b[ob]) / unit);
			}
		}
	}
	t.bounded += bounded;
}

std::vector<float> padded(uint32_t dim) {
	return std::vector<float>((dim + 3) / 4 * 4, 0.f);
}

int run_bound(int metric, uint32_t dim, uint64_t pairs, uint64_t seed) {
	std::mt19937_64 rng(seed);
	std::normal_distribution<float> gauss(0.f, 1.f);
	std::uniform_int_distribution<int> small(-127, 127);
	const float unit = 1.0f / std::sqrt((float)dim);
	const char *names[] = {"random", "near", "multiples", "tiny_rows", "huge_rows", "tiny_queries", "huge_both", "dominant", "small_rows", "large_both"};
	for (int cs = 0; cs != 10; ++cs) {
		Tally t;
		for (uint64_t p = 0; p != pairs; ++p) {
			std::vector<float> q = padded(dim), x = padded(dim);
			for (uint32_t i = 0; i != dim; ++i)
				q[i] = gauss(rng) * unit, x[i] = gauss(rng) * unit;
			if (cs == 1) // the query next to the row: distances near zero, where the bound is tightest
				for (uint32_t i = 0; i != dim; ++i)
					q[i] = x[i] + 0.05f * q[i];
			if (cs == 2) { // exact multiples of the scale: err = 0, whatever error there is is the slack's to cover
				const float s = std::ldexp(1.0f + (float)(rng() % 1024) / 1024.0f, -8);
				for (uint32_t i = 0; i != dim; ++i)
					x[i] = s * (float)small(rng);
				x[rng() % dim] = s * 127.f;
				if (p & 1) // half of them with the query equal to the row
					q = x;
			}
			// 1e-18 and 1e+18 leave the range in which the bound is given at all (norms of 2^-40 .. 2^40): the property must hold
			// all the same; 1e-9 and 1e+9 are inside it
			const float row_scale = cs == 3 ? 1e-18f : (cs == 4 || cs == 6) ? 1e18f : cs == 8 ? 1e-9f : cs == 9 ? 1e9f : 1.f;
			const float query_scale = cs == 5 ? 1e-18f : cs == 6 ? 1e18f : cs == 9 ? 1e9f : 1.f;
			for (uint32_t i = 0; i != dim; ++i)
				x[i] *= row_scale, q[i] *= query_scale;
			if (cs == 7)
				x[rng() % dim] = (p & 1 ? -1.f : 1.f) * 100.f * unit * (1.f + gauss(rng) * gauss(rng));
			check_pair(metric, dim, q, x, t);
		}
		std::printf("%s %llu %llu %llu %.9g\n", names[cs], (unsigned long long)t.pairs, (unsigned long long)t.violations,
		            (unsigned long long)t.bounded, t.worst);
	}
	return 0;
}

int run_degenerate(int metric, uint32_t dim) {
	std::mt19937_64 rng(99);
	std::normal_distribution<float> gauss(0.f, 1.f);
	std::vector<float> good = padded(dim);
	for (uint32_t i = 0; i != dim; ++i)
		good[i] = gauss(rng);
	auto with = [&](float v, bool all) {
		std::vector<float> r = all ? padded(dim) : good;
		if (all)
			for (uint32_t i = 0; i != dim; ++i)
				r[i] = v;
		else
			r[dim / 3] = v;
		return r;
	};
	struct Case {
		const char *name;
		std::vector<float> q, x;
	};
	const Case cases[] = {
	    {"zero_row", good, with(0.f, true)},          {"denormal_row", good, with(1e-42f, true)},
	    {"inf_row", good, with(INFINITY, false)},     {"minus_inf_row", good, with(-INFINITY, false)},
	    {"nan_row", good, with(NAN, false)},          {"zero_query", with(0.f, true), good},
	    {"denormal_query", with(1e-42f, true), good}, {"inf_query", with(INFINITY, false), good},
	    {"nan_query", with(NAN, false), good},        {"control", good, good},
	};
	for (const Case &c : cases) {
		const Encoded e = encode(c.x);
		bool bounded = false, violated = false;
		for (int o = 0; o != 3; ++o) {
			const float b = bound_in(metric, o, c.q, e, dim), d = engine_distance(metric, o, c.q, c.x);
			bounded = bounded || b > -INFINITY;
			violated = violated || b > d || (d != d && b > -INFINITY);
		}
		std::printf("%s %d %d\n", c.name, bounded ? 1 : 0, violated ? 1 : 0);
	}
	return 0;
}

int run_residual(uint32_t dim, uint64_t rows, uint64_t seed) {
	std::mt19937_64 rng(seed);
	std::normal_distribution<float> gauss(0.f, 1.f);
	uint64_t violations = 0;
	for (uint64_t r = 0; r != rows; ++r) {
		std::vector<float> x = padded(dim);
		const float mag = std::ldexp(1.f, (int)(rng() % 80) - 40);
		for (uint32_t i = 0; i != dim; ++i)
			x[i] = gauss(rng) * mag * ((r % 3) == 0 && (i % 7) ? 0.01f : 1.f);
		const Encoded e = encode(x);
		long double e2 = 0;
		for (size_t i = 0; i != x.size(); ++i) {
			const long double d = (long double)x[i] - (long double)e.meta.scale * (long double)e.code[i];
			e2 += d * d;
		}
		violations += !((long double)e.meta.err >= sqrtl(e2));
		violations += !(e.meta.err <= 1.001f * (float)sqrtl(e2) + 1e-30f); // (and not padded beyond its stated margin)
		for (size_t i = 0; i != x.size(); ++i)
			violations += e.code[i] < -127; // -128 is never written
	}
	std::printf("%llu %llu\n", (unsigned long long)rows, (unsigned long long)violations);
	return 0;
}

// StaleSlots against a bitmap: every marked slot below `rows` is inside the range take() hands out, every other marked slot
// stays covered by what the structure keeps
int run_stale(uint64_t rounds, uint64_t seed) {
	std::mt19937_64 rng(seed);
	uint64_t violations = 0;
	for (uint64_t r = 0; r != rounds; ++r) {
		const uint64_t cap = 64;
		std::vector<char> stale(cap, 0);
		bool all_beyond = false; // mark_all also covers slots beyond cap
		StaleSlots s;
		for (int step = 0; step != 40; ++step) {
			const int op = (int)(rng() % 8);
			if (op < 4) {
				uint64_t a = rng() % cap, b = rng() % (cap + 1);
				if (op == 0)
					b = a; // an empty range marks nothing
				for (uint64_t i = a; i < b; ++i)
					stale[i] = 1;
				s.mark(a, b);
			} else if (op == 4) {
				std::fill(stale.begin(), stale.end(), 1);
				all_beyond = true;
				s.mark_all();
			} else {
				const uint64_t rows = rng() % (cap + 1);
				uint64_t first = 0, end = 0;
				const bool work = s.take(rows, first, end);
				for (uint64_t i = 0; i != rows; ++i) {
					violations += stale[i] && !(work && first <= i && i < end);
					stale[i] = 0;
				}
				violations += work && end > rows;
			}
			for (uint64_t i = 0; i != cap; ++i)
				violations += stale[i] && !(s.lo <= i && i < s.hi);
			violations += all_beyond && !(s.any() && s.hi > cap);
		}
	}
	std::printf("%llu %llu\n", (unsigned long long)rounds, (unsigned long long)violations);
	return 0;
}

} // namespace

int main(int argc, char **argv) {
	const std::string mode = argc > 1 ? argv[1] : "";
	auto arg = [&](int i) { return i < argc ? std::strtoull(argv[i], nullptr, 10) : 0ull; };
	if (mode == "bound" && argc == 6)
		return run_bound((int)arg(2), (uint32_t)arg(3), arg(4), arg(5));
	if (mode == "degenerate" && argc == 4)
		return run_degenerate((int)arg(2), (uint32_t)arg(3));
	if (mode == "residual" && argc == 5)
		return run_residual((uint32_t)arg(2), arg(3), arg(4));
	if (mode == "stale" && argc == 4)
		return run_stale(arg(2), arg(3));
	std::fprintf(stderr, "usage: prescore_probe bound|degenerate|residual|stale ...\n");
	return 2;
}
