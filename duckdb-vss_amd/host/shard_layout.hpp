// shard_layout.hpp — which shard owns a row, and the header of a persisted sharded index.  Pure arithmetic: no HIP, no
// vssgpu.h, so it compiles with a plain C++17 compiler and is checked on the CPU (shard_layout_check.cpp).
// sharded_index.hpp routes every row and frames its container through this file; duckdb-vss_amd/sharded.py route_row is
// the same rule for the multi-process flavour.
//
// Routing rule.  G = number of shards, n_total = the row count the index was bulk-built with (0 is legal: the index is
// created empty and every row is inserted), B = 2048 = STANDARD_VECTOR_SIZE:
//   * rowid < 0          refused (std::invalid_argument here; ShardedHNSWIndex turns it into its InternalException);
//   * rowid < n_total    the row-range owner: shard g owns [g*n_total/G, (g+1)*n_total/G) (ShardRange);
//   * rowid >= n_total   ((rowid - n_total) / B) mod G — block-cyclic.  DuckDB appends rows with consecutive ids in chunks of
//                        at most 2048, so a chunk falls into one or two shards and consecutive chunks go round the shards;
//                        after any number of consecutive inserts the loads of two shards differ by at most B rows.
// The rule is stateless: Delete routes by the same function, and no rowid -> shard map is kept or persisted.  What it needs
// — G, n_total, B — is in the container header.
//
// Container, little-endian: magic "VSSSHRD1", u32 version = 1, u32 G, u64 n_total, u64 dim, u64 route block B
// (HEADER_BYTES = 40); then for each shard in order: u64 stream length, and that many bytes of the shard's usearch stream
// exactly as vss_save writes it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>

namespace vss_host {
namespace shard_layout {

constexpr uint64_t ROUTE_BLOCK = 2048; // STANDARD_VECTOR_SIZE
constexpr uint32_t CONTAINER_VERSION = 1;
constexpr size_t HEADER_BYTES = 40;
constexpr char MAGIC[9] = "VSSSHRD1";

// rows [first, second) of shard g: contiguous, disjoint, covering [0, n_total), sizes differ by at most one
inline std::pair<uint64_t, uint64_t> ShardRange(uint64_t g, uint64_t n_shards, uint64_t n_total) {
	return {g * n_total / n_shards, (g + 1) * n_total / n_shards};
}

// owner of a row inside the build's range (rowid < n_total)
inline uint64_t RangeOwner(uint64_t rowid, uint64_t n_shards, uint64_t n_total) {
	uint64_t g = rowid * n_shards / n_total;
	if (g > n_shards - 1)
		g = n_shards - 1;
	while (g > 0 && rowid < ShardRange(g, n_shards, n_total).first)
		g--;
	while (g + 1 < n_shards && rowid >= ShardRange(g, n_shards, n_total).second)
		g++;
	return g;
}

inline uint64_t OwnerOf(int64_t rowid, uint64_t n_shards, uint64_t n_total, uint64_t route_block = ROUTE_BLOCK) {
	if (rowid < 0)
		throw std::invalid_argument("negative row id " + std::to_string(rowid) + " has no shard");
	if (!n_shards || !route_block)
		throw std::invalid_argument("routing needs at least one shard and a route block of at least one row");
	if ((uint64_t)rowid < n_total)
		return RangeOwner((uint64_t)rowid, n_shards, n_total);
	return (((uint64_t)rowid - n_total) / route_block) % n_shards;
}

struct ContainerHeader {
	uint32_t version = CONTAINER_VERSION;
	uint32_t n_shards = 0;
	uint64_t n_total = 0;
	uint64_t dim = 0;
	uint64_t route_block = ROUTE_BLOCK;
};

inline void PutLE(uint8_t *out, uint64_t v, size_t bytes) {
	for (size_t i = 0; i != bytes; ++i)
		out[i] = (uint8_t)(v >> (8 * i));
}
inline uint64_t GetLE(const uint8_t *in, size_t bytes) {
	uint64_t v = 0;
	for (size_t i = 0; i != bytes; ++i)
		v |= (uint64_t)in[i] << (8 * i);
	return v;
}

inline void Encode(const ContainerHeader &h, uint8_t out[HEADER_BYTES]) {
	std::memcpy(out, MAGIC, 8);
	PutLE(out + 8, h.version, 4);
	PutLE(out + 12, h.n_shards, 4);
	PutLE(out + 16, h.n_total, 8);
	PutLE(out + 24, h.dim, 8);
	PutLE(out + 32, h.route_block, 8);
}

// "" on success, else what is wrong with the first `size` bytes at `in` as a container header
inline std::string Decode(const uint8_t *in, size_t size, ContainerHeader &h) {
	if (size < HEADER_BYTES)
		return "container header is " + std::to_string(size) + " bytes, " + std::to_string(HEADER_BYTES) + " needed";
	if (std::memcmp(in, MAGIC, 8) != 0)
		return "magic mismatch: not a sharded index container";
	ContainerHeader r;
	r.version = (uint32_t)GetLE(in + 8, 4);
	r.n_shards = (uint32_t)GetLE(in + 12, 4);
	r.n_total = GetLE(in + 16, 8);
	r.dim = GetLE(in + 24, 8);
	r.route_block = GetLE(in + 32, 8);
	if (r.version != CONTAINER_VERSION)
		return "container version " + std::to_string(r.version) + ", this code reads version " +
		       std::to_string(CONTAINER_VERSION);
	if (!r.n_shards)
		return "container names zero shards";
	if (!r.route_block)
		return "container names a route block of zero rows";
	h = r;
	return "";
}

} // namespace shard_layout
} // namespace vss_host
