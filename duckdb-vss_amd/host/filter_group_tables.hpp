// filter_group_tables.hpp — how a join chunk with a correlated predicate becomes the arguments of
// vss_search_batch_filtered_groups: one bitmap over row ids per distinct predicate value, laid end to end, and the number of
// its bitmap for every outer row.  Pure C++ (no HIP, no engine): filter_groups_harness.cpp drives the engine with it,
// filter_groups_check.cpp checks it on a CPU under the sanitizers.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

namespace vss_host {

struct FilterGroupTables {
	uint64_t n_groups = 0, n_bits = 0, words = 0; // words per group = (n_bits + 63) / 64
	std::vector<uint64_t> allowed;                // n_groups x words
	std::vector<uint32_t> group_of;               // one group per query

	FilterGroupTables(uint64_t groups, uint64_t bits) : n_groups(groups), n_bits(bits), words((bits + 63) / 64) {
		allowed.assign(n_groups * words, 0);
	}
	const uint64_t *Group(uint64_t g) const {
		return allowed.data() + g * words;
	}
	void Admit(uint64_t g, uint64_t rowid) {
		if (g < n_groups && rowid < n_bits)
			allowed[g * words + (rowid >> 6)] |= 1ull << (rowid & 63);
	}
	// every word of the group all ones — the padding after n_bits included, which must admit nothing
	void AdmitAllWithPadding(uint64_t g) {
		for (uint64_t w = 0; w != words; ++w)
			allowed[g * words + w] = ~0ull;
	}
	bool Admits(uint64_t g, int64_t rowid) const {
		return rowid >= 0 && (uint64_t)rowid < n_bits && ((Group(g)[(uint64_t)rowid >> 6] >> ((uint64_t)rowid & 63)) & 1);
	}
	// the positions of the queries of group g, in query order: what a caller without the grouped call launches one by one
	std::vector<uint64_t> QueriesOf(uint64_t g) const {
		std::vector<uint64_t> at;
		for (uint64_t q = 0; q != group_of.size(); ++q)
			if (group_of[q] == g)
				at.push_back(q);
		return at;
	}
};

// the tenant of a row: a fixed scramble of its id, so that the tenants interleave everywhere in the graph
inline uint64_t TenantOf(uint64_t rowid, uint64_t n_tenants) {
	uint64_t x = rowid * 0x9E3779B97F4A7C15ull;
	x ^= x >> 29;
	return x % n_tenants;
}

// `n_tenants` disjoint groups (WHERE items.tenant = q.tenant) over the rows `live` lets through, then one all-ones group
// (padding set); query q belongs to group q % (n_tenants + 1), so neighbouring queries never share a predicate
inline FilterGroupTables TenantTables(uint64_t n_tenants, uint64_t n_bits, uint64_t n_queries,
                                      const std::function<bool(uint64_t)> &live) {
	FilterGroupTables t(n_tenants + 1, n_bits);
	for (uint64_t id = 0; id != n_bits; ++id)
		if (live(id))
			t.Admit(TenantOf(id, n_tenants), id);
	t.AdmitAllWithPadding(n_tenants);
	t.group_of.resize(n_queries);
	for (uint64_t q = 0; q != n_queries; ++q)
		t.group_of[q] = (uint32_t)(q % (n_tenants + 1));
	return t;
}

// rows `at` of a row-major n x width array, packed
template <class T>
std::vector<T> GatherRows(const T *rows, uint64_t width, const std::vector<uint64_t> &at) {
	std::vector<T> out(at.size() * width);
	for (uint64_t i = 0; i != at.size(); ++i)
		std::memcpy(out.data() + i * width, rows + at[i] * width, width * sizeof(T));
	return out;
}

// cell by cell: rows `at` of the grouped call's answers against the packed answers of one per-group call (bit patterns:
// distances are compared as the 32 bits they are).  Returns the first differing query, or -1.
template <class T>
int64_t FirstDifference(const T *grouped, const T *per_group, uint64_t width, const std::vector<uint64_t> &at) {
	for (uint64_t i = 0; i != at.size(); ++i)
		if (std::memcmp(grouped + at[i] * width, per_group + i * width, width * sizeof(T)))
			return (int64_t)at[i];
	return -1;
}

} // namespace vss_host
