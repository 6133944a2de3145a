// shard_layout_check.cpp — CPU check of shard_layout.hpp (routing rule, container header).  Includes nothing else of the
// project, needs no GPU:
//     g++ -std=c++17 -fsanitize=address,undefined shard_layout_check.cpp -o shard_layout_check && ./shard_layout_check
//     ./shard_layout_check --table     prints "rowid G n_total owner" for the whole grid (compared with sharded.route_row)
// Exit code 0 and a last line "shard layout ok" = every check passed.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "shard_layout.hpp"

using namespace vss_host::shard_layout;

#define EXPECT(cond)                                                                                                   \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			std::fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                               \
			return 1;                                                                                                  \
		}                                                                                                              \
	} while (0)

static const uint64_t kShards[] = {1, 2, 3, 8};
static const uint64_t kTotals[] = {0, 1, 7, 6001};
static const uint64_t kInserted = 3 * ROUTE_BLOCK + 1; // three full route blocks plus one extra row

static bool Refuses(int64_t rowid, uint64_t G, uint64_t n) {
	try {
		(void)OwnerOf(rowid, G, n);
	} catch (const std::invalid_argument &) {
		return true;
	}
	return false;
}

static int Table() {
	for (uint64_t G : kShards)
		for (uint64_t n : kTotals)
			for (uint64_t r = 0; r != n + kInserted; ++r)
				std::printf("%llu %llu %llu %llu\n", (unsigned long long)r, (unsigned long long)G, (unsigned long long)n,
				            (unsigned long long)OwnerOf((int64_t)r, G, n));
	return 0;
}

int main(int argc, char **argv) {
	if (argc > 1 && std::string(argv[1]) == "--table")
		return Table();
	for (uint64_t G : kShards)
		for (uint64_t n : kTotals) {
			// the ranges cover [0, n) without gaps, and every in-range row belongs to the shard whose range holds it
			uint64_t covered = 0;
			for (uint64_t g = 0; g != G; ++g) {
				const auto r = ShardRange(g, G, n);
				EXPECT(r.first == covered && r.second >= r.first);
				covered = r.second;
				for (uint64_t row = r.first; row != r.second; ++row)
					EXPECT(OwnerOf((int64_t)row, G, n) == g);
			}
			EXPECT(covered == n);
			// ids past the build's range: block-cyclic, checked row by row (so on both sides of every block edge) ...
			for (uint64_t j = 0; j != kInserted; ++j)
				EXPECT(OwnerOf((int64_t)(n + j), G, n) == (j / ROUTE_BLOCK) % G);
			// ... and once more, spelled out, for the two rows at every edge
			for (uint64_t b = 1; b * ROUTE_BLOCK < kInserted; ++b) {
				EXPECT(OwnerOf((int64_t)(n + b * ROUTE_BLOCK - 1), G, n) == (b - 1) % G);
				EXPECT(OwnerOf((int64_t)(n + b * ROUTE_BLOCK), G, n) == b % G);
			}
			EXPECT(OwnerOf((int64_t)n, G, n) == 0);
			// negative ids have no owner
			EXPECT(Refuses(-1, G, n) && Refuses(INT64_MIN, G, n) && !Refuses(0, G, n));
			// after R consecutive inserted ids no shard is more than one route block ahead of another
			for (uint64_t R : {uint64_t(1), ROUTE_BLOCK - 1, ROUTE_BLOCK, ROUTE_BLOCK + 1, 5 * ROUTE_BLOCK + 100}) {
				std::vector<uint64_t> load(G, 0);
				for (uint64_t j = 0; j != R; ++j)
					load[OwnerOf((int64_t)(n + j), G, n)]++;
				const auto mm = std::minmax_element(load.begin(), load.end());
				EXPECT(*mm.second - *mm.first <= ROUTE_BLOCK);
				uint64_t sum = 0;
				for (uint64_t l : load)
					sum += l;
				EXPECT(sum == R);
			}
		}

	// the header round-trips, byte layout as documented
	ContainerHeader h;
	h.n_shards = 8, h.n_total = 0x0102030405060708ull, h.dim = 768, h.route_block = ROUTE_BLOCK;
	uint8_t buf[HEADER_BYTES];
	Encode(h, buf);
	EXPECT(!std::memcmp(buf, "VSSSHRD1", 8));
	EXPECT(buf[8] == 1 && buf[9] == 0 && buf[12] == 8 && buf[16] == 0x08 && buf[23] == 0x01); // little-endian
	EXPECT(buf[24] == 0x00 && buf[25] == 0x03 && buf[32] == 0x00 && buf[33] == 0x08);
	ContainerHeader back;
	EXPECT(Decode(buf, HEADER_BYTES, back).empty());
	EXPECT(back.version == 1 && back.n_shards == 8 && back.n_total == h.n_total && back.dim == 768 &&
	       back.route_block == ROUTE_BLOCK);
	{ // longer buffers are fine: the streams follow
		std::vector<uint8_t> longer(buf, buf + HEADER_BYTES);
		longer.resize(HEADER_BYTES + 100, 0xAB);
		EXPECT(Decode(longer.data(), longer.size(), back).empty());
	}
	// refusals: each says why, and leaves the output header alone
	auto refused = [&](const std::vector<uint8_t> &bytes) {
		ContainerHeader out;
		out.n_shards = 77;
		const std::string why = Decode(bytes.data(), bytes.size(), out);
		return !why.empty() && out.n_shards == 77;
	};
	const std::vector<uint8_t> good(buf, buf + HEADER_BYTES);
	{
		auto bad = good;
		bad[3] ^= 0x20; // magic
		EXPECT(refused(bad));
	}
	{
		ContainerHeader v2 = h;
		v2.version = 2;
		std::vector<uint8_t> bad(HEADER_BYTES);
		Encode(v2, bad.data());
		EXPECT(refused(bad));
	}
	{
		// one byte short: a heap copy of exactly that size, so a read past it is an AddressSanitizer report
		std::vector<uint8_t> bad(good.begin(), good.end() - 1);
		bad.shrink_to_fit();
		EXPECT(refused(bad));
		EXPECT(refused(std::vector<uint8_t>()));
	}
	{
		ContainerHeader g0 = h;
		g0.n_shards = 0;
		std::vector<uint8_t> bad(HEADER_BYTES);
		Encode(g0, bad.data());
		EXPECT(refused(bad));
	}
	{
		ContainerHeader b0 = h;
		b0.route_block = 0;
		std::vector<uint8_t> bad(HEADER_BYTES);
		Encode(b0, bad.data());
		EXPECT(refused(bad));
	}
	std::printf("shard layout ok\n");
	return 0;
}
