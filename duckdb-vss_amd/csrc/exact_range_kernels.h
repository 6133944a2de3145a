// exact_range_kernels.h — exact RANGE search: every live row within a per-query radius (vss_search_range_batch).
//
//   k_range_prepare      per query: E from the cached norm extrema (exact_certificate.h), the score threshold theta_q
//                        (exact_range.h); clears the query's count and cursor
//   k_range_candidates   one launch per (query block, row chunk): Q . X^T on v_mfma_f32_32x32x2_f32, 128 queries x 128 rows per
//                        workgroup; the epilogue keeps the (query, slot) pairs with !(score > theta_q), compacts them in LDS and
//                        appends them to the launch's candidate buffer with ONE global atomic per workgroup
//   k_range_candidates_lists   the same tile with its B operand GATHERED through a list of slots, for the range search under
//                        per-query label boxes (vss_search_range_batch_by_label_box64): one workgroup per tile of a plan
//                        (range_filtered_plan.h) and run of list positions, in two shapes, 128 queries x 128 listed rows and
//                        32 queries x 256 listed rows
//   k_range_candidates_bf16x3, k_range_candidates_lists_bf16x3   both tiles on the bf16 matrix pipe (option range.split_bf16,
//                        score kind 1: exact_range_split_kernels.h)
//   k_range_candidates_i8, k_range_candidates_lists_i8   both tiles on the int8 matrix pipe over the 8-bit row codes (option
//                        range.codes_i8, score kind 2: exact_range_codes_kernels.h, defined in exact_range_codes.hip)
//   k_range_rescore     64 / G candidates side by side per wave, four deep: the wave-order metric itself (accumulate4,
//                        group_butterfly, finish_distance: the bits of k_exact_rerank), d <= r, the per-query count, and the
//                        (query, row id, d) triple into the match scratch while the caller's capacity lasts
//   k_range_offsets      counts -> offsets (one workgroup, 64-bit)
//   k_range_scatter      the triples into the caller's cells, per-query cursors; nothing if the total exceeds the capacity
//
// Nothing overflows and nothing is re-run: a launch of the tile covers at most RANGE_QUERY_BLOCK x RANGE_ROW_CHUNK pairs and the
// candidate buffer holds that many; a workgroup's LDS compaction buffer holds all 128 x 128 pairs of its tile.
//
// The kernels are defined once, in exact_range.hip (a translation unit of its own: built without packed f32 arithmetic, and
// the engine's build time stays what it was); the engine calls the launchers below.
#pragma once
#include "exact_kernels.h"
#include "exact_range.h"
#include "range_filtered_plan.h"

namespace vss {

struct RangeStats { // device words of one call
	unsigned long long candidates, matches, no_bound;
	unsigned long long e_max; // bit pattern of the largest finite E of k_range_prepare (non-negative doubles order as their bits)
};

struct RangePrepareArgs {
	int metric;
	int score_kind;          // whose error bound the thresholds carry: 0 = the f32 tiles, 1 = the split-bf16 tiles
	uint32_t n;              // padded dimension
	uint32_t n_queries;
	const float *radii;
	const float *query_norm2; // wave-order sums of squares of the padded queries (k_row_norms)
	const uint32_t *norm_ext; // k_norm_extrema
	float *theta;
	uint32_t *counts, *cursors;
	RangeStats *stats;
};

struct RangeTileArgs {
	const float4 *queries; // n_queries x V float4 (zero padded)
	const float4 *vectors; // rows x V float4
	const float *row_norm2;
	const int64_t *keys;
	const float *theta;
	uint32_t V;
	uint32_t q_begin, q_end;     // the launch's queries ...
	uint32_t row_begin, row_end; // ... and rows: (q_end - q_begin) * (row_end - row_begin) <= the cells of `cand`
	int metric;
	uint2 *cand;          // (query, slot)
	uint32_t *cand_count; // this launch's own word, zero before it
};

// one launch of a plan (host::RangeFilterLaunch) in one of its two shapes: workgroup row y takes tile tiles[tile_index[y]]
struct RangeListTileArgs {
	const float4 *queries; // n_queries x V float4 (zero padded), by ORIGINAL query index
	const float4 *vectors;
	const float *row_norm2;
	const float *theta;    // by original query index
	const uint32_t *order; // the group order: position -> original query index
	const uint32_t *lists; // the pass's lists of live admitted slots
	const host::ExactFilterTile *tiles;
	const uint32_t *tile_index;
	uint32_t n_tiles;
	uint32_t V;
	uint32_t pos_begin, pos_end; // of every tile's list; sum over the tiles of n_queries x positions <= the cells of `cand`
	int metric;
	uint2 *cand;          // (original query index, slot)
	uint32_t *cand_count; // this launch's own word, zero before its first shape
};

struct RangeRescoreArgs {
	RowSpace sp;
	const int64_t *keys;
	const float4 *queries; // padded, as the tile's
	const float *query_norm2;
	const float *radii;
	const uint2 *cand;
	const uint32_t *cand_count;
	uint32_t *counts;
	RangeStats *stats;
	unsigned long long capacity; // cells of the match scratch
	uint32_t *m_query;
	int64_t *m_rowid;
	float *m_dist;
	bool slots = false; // m_rowid takes the match's SLOT, not its row id: the exact search by bounds (exact_codes_kernels.h) ranks by slot
};

struct RangeLayoutArgs {
	uint32_t n_queries;
	const uint32_t *counts;
	uint32_t *cursors;
	const RangeStats *stats;
	unsigned long long capacity;
	unsigned long long *offsets; // n_queries + 1
	unsigned long long *total;
	const uint32_t *m_query;
	const int64_t *m_rowid;
	const float *m_dist;
	int64_t *out_rowids;
	float *out_dist;
};

hipError_t launch_range_prepare(const RangePrepareArgs &a, hipStream_t stream);
hipError_t launch_range_candidates(const RangeTileArgs &a, hipStream_t stream);
hipError_t launch_range_candidates_lists(const RangeListTileArgs &a, bool small, hipStream_t stream); // small: the 32-query shape
hipError_t launch_range_rescore(const RangeRescoreArgs &a, uint32_t n_cus, hipStream_t stream);
hipError_t launch_range_layout(const RangeLayoutArgs &a, uint32_t n_cus, hipStream_t stream); // offsets, then the scatter

#ifdef VSS_EXACT_RANGE_TU

__global__ __launch_bounds__(256) void k_range_prepare(RangePrepareArgs a) {
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= a.n_queries)
		return;
	const float qn2 = a.query_norm2[q];
	const double E = exact_cert_error_of(a.score_kind, a.metric, a.n, qn2, __uint_as_float(a.norm_ext[0]), __uint_as_float(a.norm_ext[1]));
	a.theta[q] = range_score_threshold(a.metric, a.radii[q], qn2, E);
	a.counts[q] = 0u, a.cursors[q] = 0u;
	if (!(E < (double)__builtin_inff()))
		atomicAdd(&a.stats->no_bound, 1ull);
	else
		atomicMax(&a.stats->e_max, (unsigned long long)__double_as_longlong(E));
}

// ---------------------------------------------------------------------------------------------------------
// The candidate tile.  256 threads = 4 waves as 2 x 2, 64 queries x 64 rows each = 2 x 2 accumulators of v_mfma_f32_32x32x2_f32.
// Operand staging, K step 32 floats:
//   * an operand image of a step is 128 rows x 128 bytes with NO padding, chunk c of row r at position c ^ (r & 7): the eight
//     lanes that stage a row write its 128 bytes as one line (a wave covers 1 KiB of contiguous LDS per ds_write_b128: every bank
//     once), and the MFMA side's ds_read_b128 of chunk 2 g + (lane >> 5) of rows lane & 31 spreads over all banks as well;
//   * two images per operand (64 KiB in all -> two workgroups per compute unit), ONE barrier per step: the registers that were
//     loaded during step k - 1 are written to the idle buffer at the top of step k, the loads of step k + 2 go out behind them
//     and stay in flight during the step's 64 MFMAs;
//   * a lane's float4 feeds four consecutive MFMAs: the two half-waves own k = 8 g + 4 h .. + 3 of every group of eight, on both
//     operands alike (a dot product does not care which k a half-wave supplies), so nothing is transposed anywhere;
//   * any V: a step beyond the row's last chunk stages zeros.
// Epilogue: once the last step's barrier has passed the operand images are dead, and their LDS becomes the compaction buffer — a
// 16-bit code (query in tile << 7 | row in tile) per surviving pair, 32 KiB when every pair survives.  A wave reserves room in it
// with one LDS atomic per ballot; the workgroup then reserves n cells of the launch's candidate buffer with one global atomic
// and writes the n (query, slot) pairs side by side.
constexpr uint32_t RT_IMAGE_BYTES = 128 * 128;
constexpr uint32_t RT_LDS_BYTES = 4 * RT_IMAGE_BYTES; // [buffer][A | B]

template <int MT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_range_candidates(RangeTileArgs a) {
	extern __shared__ __attribute__((aligned(16))) unsigned char rt_smem[];
	__shared__ float theta_l[128];
	__shared__ uint32_t n_staged, g_base;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = tid >> 6;
	const int wm = wave >> 1, wn = wave & 1;
	const uint32_t q0 = a.q_begin + blockIdx.y * 128u, r0 = a.row_begin + blockIdx.x * 128u;
	if (tid < 128)
		theta_l[tid] = q0 + tid < a.q_end ? a.theta[q0 + tid] : -__builtin_inff();
	if (tid == 0)
		n_staged = 0u;

	f32x16 acc[2][2];
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[i][j][e] = 0.f;

	// the load side: thread -> chunk f of the step's eight, rows rr + 32 p of both operands (rows beyond the edge re-read the last)
	const uint32_t f = (uint32_t)tid & 7u, rr = (uint32_t)tid >> 3;
	const float4 *qsrc[4], *xsrc[4];
#pragma unroll
	for (int p = 0; p < 4; ++p) {
		uint32_t qi = q0 + rr + 32u * p, ri = r0 + rr + 32u * p;
		qi = qi < a.q_end ? qi : a.q_end - 1u;
		ri = ri < a.row_end ? ri : a.row_end - 1u;
		qsrc[p] = a.queries + (size_t)qi * a.V;
		xsrc[p] = a.vectors + (size_t)ri * a.V;
	}
	const uint32_t steps = (a.V + 7u) / 8u;
	float4 qa[4], xb[4];
	auto load_step = [&](uint32_t step) { // unconditional (clamped chunk, zeroed afterwards): guarded loads are waited for one by one
		const uint32_t c = step * 8u + f, cc = c < a.V ? c : a.V - 1u;
#pragma unroll
		for (int p = 0; p < 4; ++p)
			qa[p] = qsrc[p][cc], xb[p] = xsrc[p][cc];
		if (c >= a.V) {
#pragma unroll
			for (int p = 0; p < 4; ++p)
				qa[p] = xb[p] = make_float4(0.f, 0.f, 0.f, 0.f);
		}
	};
	const uint32_t st_off = rr * 128u + ((f ^ (rr & 7u)) << 4); // (rows rr + 32 p: the same row & 7)
	auto store_step = [&](int buf) {
		unsigned char *A = rt_smem + buf * 2 * RT_IMAGE_BYTES, *B = A + RT_IMAGE_BYTES;
#pragma unroll
		for (int p = 0; p < 4; ++p) {
			*reinterpret_cast<float4 *>(A + st_off + p * 32 * 128) = qa[p];
			*reinterpret_cast<float4 *>(B + st_off + p * 32 * 128) = xb[p];
		}
	};
	// the MFMA side: row lane & 31 of each 32-row tile, chunk 2 g + (lane >> 5) of k-group g
	const uint32_t a_row = (uint32_t)(wm * 64 + (lane & 31)) * 128u, b_row = RT_IMAGE_BYTES + (uint32_t)(wn * 64 + (lane & 31)) * 128u;
	uint32_t pos[4];
#pragma unroll
	for (int g = 0; g < 4; ++g)
		pos[g] = (((uint32_t)(2 * g) + ((uint32_t)lane >> 5)) ^ ((uint32_t)lane & 7u)) << 4;
	auto read_group = [&](int buf, int g, float4 (&av)[2], float4 (&bv)[2]) {
		const unsigned char *I = rt_smem + buf * 2 * RT_IMAGE_BYTES;
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			av[i] = *reinterpret_cast<const float4 *>(I + a_row + i * 32 * 128 + pos[g]);
			bv[i] = *reinterpret_cast<const float4 *>(I + b_row + i * 32 * 128 + pos[g]);
		}
	};
	auto mfma_group = [&](const float4 (&av)[2], const float4 (&bv)[2]) {
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
	};

	load_step(0);
	store_step(0);
	if (steps > 1)
		load_step(1);
	// what the epilogue reads from memory, asked for ahead of the loop: this lane's two columns
	float col_n2[2];
	bool col_live[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t col = r0 + wn * 64 + j * 32 + (lane & 31), cc = col < a.row_end ? col : a.row_end - 1u;
		col_n2[j] = a.row_norm2[cc];
		col_live[j] = col < a.row_end && a.keys[cc] != FREE_KEY;
	}
	__syncthreads();
	for (uint32_t k = 0; k < steps; ++k) {
		const int buf = (int)(k & 1u);
		float4 av0[2], bv0[2], av1[2], bv1[2];
		read_group(buf, 0, av0, bv0);
		if (k + 1 < steps)
			store_step(buf ^ 1); // step k + 1, loaded a whole step ago; the idle buffer's readers passed the last barrier
		read_group(buf, 1, av1, bv1);
		if (k + 2 < steps)
			load_step(k + 2);
		mfma_group(av0, bv0);
		read_group(buf, 2, av0, bv0);
		mfma_group(av1, bv1);
		read_group(buf, 3, av1, bv1);
		mfma_group(av0, bv0);
		mfma_group(av1, bv1);
		__syncthreads();
	}

	// ---- epilogue: C[row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][col = lane & 31]; the operand images are dead
	uint16_t *staged = reinterpret_cast<uint16_t *>(rt_smem);
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t cl = wn * 64 + j * 32 + (lane & 31);
		const float xn2 = col_n2[j], rs = MT == 1 ? rsqrtf(xn2) : 0.f;
#pragma unroll
		for (int i = 0; i < 2; ++i) {
#pragma unroll
			for (int e = 0; e < 16; ++e) {
				const uint32_t ql = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * ((uint32_t)lane >> 5);
				const float s = exact_score<MT>(acc[i][j][e], xn2, rs);
				const bool keep = col_live[j] && q0 + ql < a.q_end && !(s > theta_l[ql]);
				const unsigned long long m = __ballot(keep);
				if (m) { // (wave-uniform)
					uint32_t base = 0;
					if (lane == 0)
						base = atomicAdd(&n_staged, (uint32_t)__popcll(m));
					base = __shfl(base, 0);
					if (keep)
						staged[base + __popcll(m & lanes_below(lane))] = (uint16_t)(ql << 7 | cl);
				}
			}
		}
	}
	__syncthreads();
	const uint32_t n = n_staged;
	if (n == 0)
		return;
	if (tid == 0)
		g_base = atomicAdd(a.cand_count, n);
	__syncthreads();
	uint2 *out = a.cand + g_base;
	for (uint32_t t = tid; t < n; t += 256) {
		const uint32_t code = staged[t];
		out[t] = make_uint2(q0 + (code >> 7), r0 + (code & 127u));
	}
}

// ---------------------------------------------------------------------------------------------------------
// The gathered candidate tile: the tile above with row r of the B operand = row lists[list_offset + pos] of the index, one
// indirection per row (a row is 16 V contiguous bytes: whole cache lines still), and query t of the A operand = query
// order[first_query + t].  A loading thread reads its list entries, and a lane of the epilogue its columns' |x|^2, ahead of the
// K loop.  Listed rows are live (the listing kernels skip FREE_KEY); positions from the end of the list or of the launch's run,
// and queries from n_queries, are padding: col_live = false, theta = -inf.  Staging, swizzle, double buffering, the single
// barrier per step, loads two steps ahead, the half-wave K split and the zero staging past V are the dense tile's.
// Two shapes, one launch each over its own tile-index array (the accumulator counts differ):
//   QH = 128  2 x 2 waves of 64 x 64: 128 queries x 128 listed rows, 2 x (16 + 16) KiB of operand images
//   QH = 32   four waves side by side along the list, 32 queries x 64 rows each (1 x 2 accumulators): 32 queries x 256 listed
//             rows, 2 x (4 + 32) KiB — a tile of a few queries wastes at most 31 query rows of MFMA instead of 127, at a
//             quarter of the flops per staged B byte
// Either way two workgroups fit a compute unit's 160 KiB.  The epilogue's code is query in tile << LOG_W | row in tile (7 + 7
// or 5 + 8 bits); the original query index and the slot of a surviving pair are read through order / lists when it is written.
template <int QH>
struct RangeListShape {
	static constexpr uint32_t W = QH == 128 ? 128 : 256, LOG_W = QH == 128 ? 7 : 8; // listed rows per workgroup
	static constexpr int WN = QH == 128 ? 2 : 4;                                     // waves along the list (4 / WN along the queries)
	static constexpr int AI = QH == 128 ? 2 : 1;                                     // accumulators of a wave along the queries (two along the list)
	static constexpr int PA = QH / 32, PB = W / 32;                                  // float4 a loading thread stages per step and operand
	static constexpr uint32_t A_BYTES = QH * 128, BUF_BYTES = (QH + W) * 128, LDS_BYTES = 2 * BUF_BYTES;
};

template <int MT, int QH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_range_candidates_lists(RangeListTileArgs a) {
	using S = RangeListShape<QH>;
	extern __shared__ __attribute__((aligned(16))) unsigned char rt_smem[];
	__shared__ float theta_l[QH];
	__shared__ uint32_t n_staged, g_base;
	const host::ExactFilterTile tile = a.tiles[a.tile_index[blockIdx.y]];
	const uint32_t end = tile.list_length < a.pos_end ? tile.list_length : a.pos_end; // of this tile's positions in the launch
	const uint32_t p0 = a.pos_begin + blockIdx.x * S::W;
	if (p0 >= end) // (uniform over the workgroup) the grid follows the launch's longest list
		return;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = tid >> 6;
	const int wm = wave / S::WN, wn = wave % S::WN;
	const uint32_t *order = a.order + tile.first_query, *list = a.lists + tile.list_offset;
	if (tid < QH)
		theta_l[tid] = (uint32_t)tid < tile.n_queries ? a.theta[order[tid]] : -__builtin_inff();
	if (tid == 0)
		n_staged = 0u;

	f32x16 acc[S::AI][2];
#pragma unroll
	for (int i = 0; i < S::AI; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[i][j][e] = 0.f;

	// the load side: thread -> chunk f of the step's eight, rows rr + 32 p of both operands (rows beyond the edge re-read the last)
	const uint32_t f = (uint32_t)tid & 7u, rr = (uint32_t)tid >> 3;
	const float4 *qsrc[S::PA], *xsrc[S::PB];
#pragma unroll
	for (int p = 0; p < S::PA; ++p) {
		const uint32_t t = rr + 32u * p;
		qsrc[p] = a.queries + (size_t)order[t < tile.n_queries ? t : tile.n_queries - 1u] * a.V;
	}
#pragma unroll
	for (int p = 0; p < S::PB; ++p) {
		const uint32_t pos = p0 + rr + 32u * p;
		xsrc[p] = a.vectors + (size_t)list[pos < end ? pos : end - 1u] * a.V;
	}
	const uint32_t steps = (a.V + 7u) / 8u;
	float4 qa[S::PA], xb[S::PB];
	auto load_step = [&](uint32_t step) { // unconditional (clamped chunk, zeroed afterwards): guarded loads are waited for one by one
		const uint32_t c = step * 8u + f, cc = c < a.V ? c : a.V - 1u;
#pragma unroll
		for (int p = 0; p < S::PA; ++p)
			qa[p] = qsrc[p][cc];
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			xb[p] = xsrc[p][cc];
		if (c >= a.V) {
#pragma unroll
			for (int p = 0; p < S::PA; ++p)
				qa[p] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
			for (int p = 0; p < S::PB; ++p)
				xb[p] = make_float4(0.f, 0.f, 0.f, 0.f);
		}
	};
	const uint32_t st_off = rr * 128u + ((f ^ (rr & 7u)) << 4); // (rows rr + 32 p: the same row & 7)
	auto store_step = [&](int buf) {
		unsigned char *A = rt_smem + buf * S::BUF_BYTES, *B = A + S::A_BYTES;
#pragma unroll
		for (int p = 0; p < S::PA; ++p)
			*reinterpret_cast<float4 *>(A + st_off + p * 32 * 128) = qa[p];
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			*reinterpret_cast<float4 *>(B + st_off + p * 32 * 128) = xb[p];
	};
	// the MFMA side: row lane & 31 of each 32-row tile, chunk 2 g + (lane >> 5) of k-group g
	const uint32_t a_row = (uint32_t)(wm * 64 + (lane & 31)) * 128u, b_row = S::A_BYTES + (uint32_t)(wn * 64 + (lane & 31)) * 128u;
	uint32_t pos[4];
#pragma unroll
	for (int g = 0; g < 4; ++g)
		pos[g] = (((uint32_t)(2 * g) + ((uint32_t)lane >> 5)) ^ ((uint32_t)lane & 7u)) << 4;
	auto read_group = [&](int buf, int g, float4 (&av)[S::AI], float4 (&bv)[2]) {
		const unsigned char *I = rt_smem + buf * S::BUF_BYTES;
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
			av[i] = *reinterpret_cast<const float4 *>(I + a_row + i * 32 * 128 + pos[g]);
#pragma unroll
		for (int j = 0; j < 2; ++j)
			bv[j] = *reinterpret_cast<const float4 *>(I + b_row + j * 32 * 128 + pos[g]);
	};
	auto mfma_group = [&](const float4 (&av)[S::AI], const float4 (&bv)[2]) {
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
	};

	load_step(0);
	store_step(0);
	if (steps > 1)
		load_step(1);
	// what the epilogue reads from memory, asked for ahead of the loop: this lane's two columns
	float col_n2[2];
	bool col_live[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t col = p0 + wn * 64 + j * 32 + (lane & 31);
		col_n2[j] = a.row_norm2[list[col < end ? col : end - 1u]];
		col_live[j] = col < end;
	}
	__syncthreads();
	for (uint32_t k = 0; k < steps; ++k) {
		const int buf = (int)(k & 1u);
		float4 av0[S::AI], bv0[2], av1[S::AI], bv1[2];
		read_group(buf, 0, av0, bv0);
		if (k + 1 < steps)
			store_step(buf ^ 1); // step k + 1, loaded a whole step ago; the idle buffer's readers passed the last barrier
		read_group(buf, 1, av1, bv1);
		if (k + 2 < steps)
			load_step(k + 2);
		mfma_group(av0, bv0);
		read_group(buf, 2, av0, bv0);
		mfma_group(av1, bv1);
		read_group(buf, 3, av1, bv1);
		mfma_group(av0, bv0);
		mfma_group(av1, bv1);
		__syncthreads();
	}

	// ---- epilogue: C[row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][col = lane & 31]; the operand images are dead, and QH x W
	// 16-bit codes (32 or 16 KiB) fit them
	uint16_t *staged = reinterpret_cast<uint16_t *>(rt_smem);
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t cl = wn * 64 + j * 32 + (lane & 31);
		const float xn2 = col_n2[j], rs = MT == 1 ? rsqrtf(xn2) : 0.f;
#pragma unroll
		for (int i = 0; i < S::AI; ++i) {
#pragma unroll
			for (int e = 0; e < 16; ++e) {
				const uint32_t ql = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * ((uint32_t)lane >> 5);
				const float s = exact_score<MT>(acc[i][j][e], xn2, rs);
				const bool keep = col_live[j] && ql < tile.n_queries && !(s > theta_l[ql]);
				const unsigned long long m = __ballot(keep);
				if (m) { // (wave-uniform)
					uint32_t base = 0;
					if (lane == 0)
						base = atomicAdd(&n_staged, (uint32_t)__popcll(m));
					base = __shfl(base, 0);
					if (keep)
						staged[base + __popcll(m & lanes_below(lane))] = (uint16_t)(ql << S::LOG_W | cl);
				}
			}
		}
	}
	__syncthreads();
	const uint32_t n = n_staged;
	if (n == 0)
		return;
	if (tid == 0)
		g_base = atomicAdd(a.cand_count, n);
	__syncthreads();
	uint2 *out = a.cand + g_base;
	for (uint32_t t = tid; t < n; t += 256) {
		const uint32_t code = staged[t];
		out[t] = make_uint2(order[code >> S::LOG_W], list[p0 + (code & (S::W - 1u))]);
	}
}

// ---------------------------------------------------------------------------------------------------------
// The re-score: lane group g of G lanes takes chunks g, g + G, ... of its candidate's row and query — the partition, fma order
// and butterfly of wave_distance_one — RR candidates deep so that their loads are in flight together.
constexpr int RANGE_RR = 4;

template <int MT>
__global__ __launch_bounds__(256) void k_range_rescore(RangeRescoreArgs a) {
	const uint32_t V = a.sp.V, G = a.sp.G;
	const uint32_t lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane >> a.sp.logG, RG = 64u >> a.sp.logG;
	const uint32_t n = *a.cand_count;
	const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
	if (wave == 0 && lane == 0)
		atomicAdd(&a.stats->candidates, (unsigned long long)n);
	for (uint32_t base = wave * RG * RANGE_RR; base < n; base += n_waves * RG * RANGE_RR) { // (wave-uniform bounds)
		uint2 c[RANGE_RR];
		const float4 *qp[RANGE_RR], *rp[RANGE_RR];
		float ab[RANGE_RR], b2[RANGE_RR];
#pragma unroll
		for (int r = 0; r < RANGE_RR; ++r) {
			const uint32_t idx = base + r * RG + sub;
			c[r] = a.cand[idx < n ? idx : n - 1u];
			qp[r] = a.queries + (size_t)c[r].x * V;
			rp[r] = a.sp.vectors + (size_t)c[r].y * V;
			ab[r] = 0.f, b2[r] = 0.f;
		}
		for (uint32_t ch = g; ch < V; ch += G) {
			float4 q[RANGE_RR], x[RANGE_RR];
#pragma unroll
			for (int r = 0; r < RANGE_RR; ++r)
				q[r] = qp[r][ch], x[r] = rp[r][ch];
#pragma unroll
			for (int r = 0; r < RANGE_RR; ++r)
				accumulate4<MT>(q[r], x[r], ab[r], b2[r]);
		}
#pragma unroll
		for (int r = 0; r < RANGE_RR; ++r) {
			const uint32_t idx = base + r * RG + sub;
			const float dot = group_butterfly(ab[r], G);
			const float xn2 = MT == 1 ? group_butterfly(b2[r], G) : 0.f;
			const float d = finish_distance<MT>(dot, MT == 1 ? a.query_norm2[c[r].x] : 0.f, xn2);
			const bool match = g == 0 && idx < n && range_matches(MT, d, a.radii[c[r].x]);
			const unsigned long long m = __ballot(match);
			if (!m) // (wave-uniform)
				continue;
			unsigned long long at = 0;
			if (lane == (uint32_t)__ffsll((long long)m) - 1u)
				at = atomicAdd(&a.stats->matches, (unsigned long long)__popcll(m));
			at = __shfl(at, __ffsll((long long)m) - 1) + (unsigned long long)__popcll(m & lanes_below((int)lane));
			if (match) {
				atomicAdd(&a.counts[c[r].x], 1u);
				if (at < a.capacity) {
					a.m_query[at] = c[r].x;
					a.m_rowid[at] = a.slots ? (int64_t)c[r].y : a.keys[c[r].y];
					a.m_dist[at] = d;
				}
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// counts -> offsets: one workgroup; thread t sums its run of queries, the runs are scanned in LDS, the thread writes its run
constexpr int RANGE_SCAN_THREADS = 1024;
__global__ __launch_bounds__(RANGE_SCAN_THREADS) void k_range_offsets(RangeLayoutArgs a) {
	__shared__ unsigned long long part[RANGE_SCAN_THREADS];
	const uint32_t t = threadIdx.x;
	const uint32_t per = (a.n_queries + RANGE_SCAN_THREADS - 1) / RANGE_SCAN_THREADS;
	const uint64_t lo = (uint64_t)t * per, hi = lo + per < a.n_queries ? lo + per : a.n_queries;
	unsigned long long sum = 0;
	for (uint64_t q = lo; q < hi; ++q)
		sum += a.counts[q];
	part[t] = sum;
	__syncthreads();
	for (uint32_t o = 1; o < RANGE_SCAN_THREADS; o <<= 1) { // inclusive scan
		const unsigned long long v = t >= o ? part[t - o] : 0ull;
		__syncthreads();
		part[t] += v;
		__syncthreads();
	}
	unsigned long long run = part[t] - sum;
	for (uint64_t q = lo; q < hi; ++q) {
		a.offsets[q] = run;
		run += a.counts[q];
	}
	if (t == RANGE_SCAN_THREADS - 1) {
		a.offsets[a.n_queries] = part[t];
		*a.total = part[t];
	}
}

__global__ __launch_bounds__(256) void k_range_scatter(RangeLayoutArgs a) {
	const unsigned long long total = a.stats->matches;
	if (total > a.capacity) // (uniform over the launch) no cell is written: the caller reads the total and calls again
		return;
	for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t q = a.m_query[i];
		const unsigned long long at = a.offsets[q] + atomicAdd(&a.cursors[q], 1u);
		a.out_rowids[at] = a.m_rowid[i];
		a.out_dist[at] = a.m_dist[i];
	}
}

// ---------------------------------------------------------------------------------------------------------
hipError_t launch_range_prepare(const RangePrepareArgs &a, hipStream_t stream) {
	hipLaunchKernelGGL(k_range_prepare, dim3((a.n_queries + 255u) / 256u), dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_range_candidates(const RangeTileArgs &a, hipStream_t stream) {
	const void *fn = a.metric == 0   ? reinterpret_cast<const void *>(k_range_candidates<0>)
	                 : a.metric == 1 ? reinterpret_cast<const void *>(k_range_candidates<1>)
	                                 : reinterpret_cast<const void *>(k_range_candidates<2>);
	if (const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RT_LDS_BYTES))
		return e;
	const dim3 grid((a.row_end - a.row_begin + 127u) / 128u, (a.q_end - a.q_begin + 127u) / 128u);
	if (a.metric == 0)
		hipLaunchKernelGGL(k_range_candidates<0>, grid, dim3(256), RT_LDS_BYTES, stream, a);
	else if (a.metric == 1)
		hipLaunchKernelGGL(k_range_candidates<1>, grid, dim3(256), RT_LDS_BYTES, stream, a);
	else
		hipLaunchKernelGGL(k_range_candidates<2>, grid, dim3(256), RT_LDS_BYTES, stream, a);
	return hipGetLastError();
}

template <int MT, int QH>
static hipError_t launch_range_candidates_lists_as(const RangeListTileArgs &a, hipStream_t stream) {
	using S = RangeListShape<QH>;
	if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_range_candidates_lists<MT, QH>),
	                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::LDS_BYTES))
		return e;
	const dim3 grid((a.pos_end - a.pos_begin + S::W - 1u) / S::W, a.n_tiles);
	hipLaunchKernelGGL((k_range_candidates_lists<MT, QH>), grid, dim3(256), S::LDS_BYTES, stream, a);
	return hipGetLastError();
}

hipError_t launch_range_candidates_lists(const RangeListTileArgs &a, bool small, hipStream_t stream) {
	if (!a.n_tiles || a.pos_begin >= a.pos_end)
		return hipSuccess;
	if (small)
		return a.metric == 0   ? launch_range_candidates_lists_as<0, 32>(a, stream)
		       : a.metric == 1 ? launch_range_candidates_lists_as<1, 32>(a, stream)
		                       : launch_range_candidates_lists_as<2, 32>(a, stream);
	return a.metric == 0   ? launch_range_candidates_lists_as<0, 128>(a, stream)
	       : a.metric == 1 ? launch_range_candidates_lists_as<1, 128>(a, stream)
	                       : launch_range_candidates_lists_as<2, 128>(a, stream);
}

hipError_t launch_range_rescore(const RangeRescoreArgs &a, uint32_t n_cus, hipStream_t stream) {
	const dim3 grid(8u * n_cus);
	if (a.sp.metric == 0)
		hipLaunchKernelGGL(k_range_rescore<0>, grid, dim3(256), 0, stream, a);
	else if (a.sp.metric == 1)
		hipLaunchKernelGGL(k_range_rescore<1>, grid, dim3(256), 0, stream, a);
	else
		hipLaunchKernelGGL(k_range_rescore<2>, grid, dim3(256), 0, stream, a);
	return hipGetLastError();
}

hipError_t launch_range_layout(const RangeLayoutArgs &a, uint32_t n_cus, hipStream_t stream) {
	hipLaunchKernelGGL(k_range_offsets, dim3(1), dim3(RANGE_SCAN_THREADS), 0, stream, a);
	if (a.capacity)
		hipLaunchKernelGGL(k_range_scatter, dim3(4u * n_cus), dim3(256), 0, stream, a);
	return hipGetLastError();
}

#endif // VSS_EXACT_RANGE_TU

} // namespace vss

#include "exact_range_split_kernels.h" // both candidate tiles on the bf16 matrix pipe (option range.split_bf16)
#include "exact_range_codes_kernels.h" // both candidate tiles on the int8 matrix pipe, over the row codes (option range.codes_i8)
