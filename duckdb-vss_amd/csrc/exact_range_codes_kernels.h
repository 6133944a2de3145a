// exact_range_codes_kernels.h — the range search's candidate tiles on the int8 matrix pipe, over the index's resident 8-bit row
// codes (option range.codes_i8, score kind 2).
//
//   k_range_prepare_codes         per query: the constants of the pair test (exact_range_codes.h) from the query's own code
//                                 record and its radius; clears the query's count and cursor, as k_range_prepare does
//   k_range_candidates_i8         k_range_candidates' 128 queries x 128 rows with  I = sum cq_i cx_i  on v_mfma_i32_32x32x32_i8:
//                                 ONE MFMA per 32 dimensions of a 32 x 32 block where the f32 tile issues sixteen, and a quarter
//                                 of the operand bytes (a row's codes are 4 V bytes, row_codes.h)
//   k_range_candidates_lists_i8   the same for k_range_candidates_lists, in its two shapes (128 x 128 and 32 x 256)
//
// The integer dot product is exact; what the codes lose is bounded per row and per query (err >= |residual|_2), and the pair test
// drops a pair only where that bound puts the engine's distance above the radius.  The tiles only PROPOSE: the re-score in the
// metric decides, so the answers are those of the f32 tiles and a loose bound costs re-scores, never answers.
//
// Included at the end of exact_range_kernels.h; the kernels are defined once, in exact_range_codes.hip.
#pragma once
#include "exact_range_codes.h"

namespace vss {

struct RangeCodesPrepareArgs {
	int metric;
	uint32_t n; // padded dimension
	uint32_t n_queries;
	const float *radii;
	const RowCodeMeta *q_meta; // k_encode_rows over the padded query block
	const uint32_t *norm_ext;  // k_norm_extrema
	RangeCodesQuery *qc;
	uint32_t *counts, *cursors;
	RangeStats *stats; // e_max: the largest finite SLACK (exact_range_codes.h)
};

// what the i8 tiles read in the place of the f32 operands
struct RangeCodesView {
	const uint32_t *q_codes;  // n_queries x V dwords, by ORIGINAL query index
	const RangeCodesQuery *qc; // by original query index
	const uint32_t *row_codes; // slots x V dwords
	const RowCodeMeta *row_meta;
};

hipError_t launch_range_prepare_codes(const RangeCodesPrepareArgs &a, hipStream_t stream);
// RangeTileArgs / RangeListTileArgs: queries, vectors, row_norm2 and theta are not read.  Both need V % 8 == 0.
hipError_t launch_range_candidates_i8(const RangeTileArgs &a, const RangeCodesView &c, hipStream_t stream);
hipError_t launch_range_candidates_lists_i8(const RangeListTileArgs &a, bool small, const RangeCodesView &c, hipStream_t stream);

#ifdef VSS_EXACT_RANGE_CODES_TU

typedef int i32x16_t __attribute__((ext_vector_type(16)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_range_prepare_codes(RangeCodesPrepareArgs a) {
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= a.n_queries)
		return;
	const RowCodeMeta qm = a.q_meta[q];
	a.qc[q] = range_codes_query(a.metric, a.n, a.radii[q], qm);
	a.counts[q] = 0u, a.cursors[q] = 0u;
	const double S = range_codes_slack(a.metric, a.n, qm, __uint_as_float(a.norm_ext[0]));
	if (!(S < (double)__builtin_inff()))
		atomicAdd(&a.stats->no_bound, 1ull);
	else
		atomicMax(&a.stats->e_max, (unsigned long long)__double_as_longlong(S));
}

// ---------------------------------------------------------------------------------------------------------
// One workgroup's tile: QH queries x W rows, 256 threads, the shapes of the f32 tiles.
//   QH = 128  2 x 2 waves of 64 x 64 (2 x 2 accumulators of sixteen i32): 128 x 128, the dense tile and the gathered tile's tall shape
//   QH = 32   four waves side by side along the rows, 32 x 64 each (1 x 2 accumulators): 32 x 256, the gathered tile's other shape
// Operand staging, K step 128 BYTES = 128 dimensions = four MFMA blocks of depth 32:
//   * an operand image of a step is rows x 128 bytes with NO padding, chunk c (16 code bytes) of row r at position c ^ (r & 7) —
//     byte for byte the f32 tile's image, so its two access patterns carry over: the eight lanes that stage a row write one
//     128-byte line, and the MFMA side's ds_read_b128 of chunk 2 kb + (lane >> 5) of rows lane & 31 — 16 bytes of K per lane and
//     MFMA, which is exactly one chunk — is the f32 tile's read of k-group kb: the eight rows that share r & 7 differ in the
//     chunk's upper bits or not at all, so every group of eight lanes covers the eight chunk positions: conflict-free;
//   * the images are as large as the f32 tile's (2 x 32 KiB, 2 x 36 KiB for the 32-query shape: two workgroups per compute
//     unit) and hold FOUR TIMES the dimensions: the room the smaller operands leave went into a deeper K step, not into
//     occupancy — a third workgroup does not fit 160 KiB beside two in any case, and with one MFMA where the f32 tile has
//     sixteen the step's barrier, its address arithmetic and the global-load round trip are what is left to hide: a step of 128
//     dimensions has a quarter of them per dimension, and loads issued two steps ahead are 256 dimensions ahead;
//   * two buffers, ONE barrier per step (an LDS-only one, so the global loads stay in flight across it): the registers loaded
//     during step k - 1 are written to the idle buffer at the top of step k, the loads of step k + 2 go out behind them;
//   * a row's codes are V / 4 chunks (V % 8 == 0: a whole number of MFMA blocks); a chunk beyond them — rows of 32, 64 or 96
//     dimensions, the last partial step — is staged as zeros: code 0 adds nothing to I;
//   * a lane supplies row lane & 31 and the sixteen k of chunk 2 kb + (lane >> 5) on both operands alike (a dot product does
//     not care which k a half-wave supplies), so nothing is transposed anywhere.
template <int QH>
struct RangeI8Shape {
	static constexpr uint32_t W = QH == 128 ? 128 : 256, LOG_W = QH == 128 ? 7 : 8; // rows per workgroup
	static constexpr int WN = W / 64;                                                // waves along the rows (4 / WN along the queries)
	static constexpr int AI = QH == 128 ? 2 : 1;                                     // accumulators of a wave along the queries (two along the rows)
	static constexpr int PA = QH / 32, PB = W / 32;                                  // chunks a loading thread stages per step and operand
	static constexpr uint32_t A_BYTES = QH * 128, BUF_BYTES = (QH + W) * 128, LDS_BYTES = 2 * BUF_BYTES;
};

// what a loading thread reads: chunk 0 of its rows (rows beyond the edge re-read the last one); a code row is V / 4 chunks
template <int QH>
struct RangeI8Sources {
	const i32x4_t *q[RangeI8Shape<QH>::PA];
	const i32x4_t *x[RangeI8Shape<QH>::PB];
};

// acc = the tile's integer dot products over the rows' V / 4 chunks.  Ends behind a barrier: the operand images are dead on return.
template <int QH>
__device__ __forceinline__ void range_i8_dots(unsigned char *smem, const RangeI8Sources<QH> &src, uint32_t chunks,
                                              i32x16_t (&acc)[RangeI8Shape<QH>::AI][2]) {
	using S = RangeI8Shape<QH>;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int wm = wave / S::WN, wn = wave % S::WN;
#pragma unroll
	for (int i = 0; i < S::AI; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[i][j][e] = 0;

	// ---- the load side: thread -> chunk f of the step's eight, rows rr + 32 p of both operands
	const uint32_t f = (uint32_t)tid & 7u, rr = (uint32_t)tid >> 3;
	const uint32_t steps = (chunks + 7u) / 8u;
	i32x4_t qa[S::PA], xb[S::PB];
	auto load_step = [&](uint32_t step) { // unconditional (clamped chunk, zeroed afterwards): guarded loads are waited for one by one
		const uint32_t c = step * 8u + f, cc = c < chunks ? c : chunks - 1u;
#pragma unroll
		for (int p = 0; p < S::PA; ++p)
			qa[p] = src.q[p][cc];
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			xb[p] = src.x[p][cc];
		if (c >= chunks) {
#pragma unroll
			for (int p = 0; p < S::PA; ++p)
				qa[p] = i32x4_t {0, 0, 0, 0};
#pragma unroll
			for (int p = 0; p < S::PB; ++p)
				xb[p] = i32x4_t {0, 0, 0, 0};
		}
	};
	const uint32_t st_off = rr * 128u + ((f ^ (rr & 7u)) << 4); // (rows rr + 32 p: the same row & 7)
	auto store_step = [&](int buf) {
		unsigned char *A = smem + buf * S::BUF_BYTES, *B = A + S::A_BYTES;
#pragma unroll
		for (int p = 0; p < S::PA; ++p)
			*reinterpret_cast<i32x4_t *>(A + st_off + p * 32 * 128) = qa[p];
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			*reinterpret_cast<i32x4_t *>(B + st_off + p * 32 * 128) = xb[p];
	};
	// ---- the MFMA side: row lane & 31 of each 32-row tile, chunk 2 kb + (lane >> 5) of block kb, at its swizzled position
	const uint32_t a_row = (uint32_t)(wm * 64 + (lane & 31)) * 128u, b_row = S::A_BYTES + (uint32_t)(wn * 64 + (lane & 31)) * 128u;
	uint32_t pos[4];
#pragma unroll
	for (int kb = 0; kb < 4; ++kb)
		pos[kb] = (((uint32_t)(2 * kb) + ((uint32_t)lane >> 5)) ^ ((uint32_t)lane & 7u)) << 4;
	auto read_block = [&](int buf, int kb, i32x4_t (&av)[S::AI], i32x4_t (&bv)[2]) {
		const unsigned char *I = smem + buf * S::BUF_BYTES + pos[kb];
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
			av[i] = *reinterpret_cast<const i32x4_t *>(I + a_row + i * 32 * 128);
#pragma unroll
		for (int j = 0; j < 2; ++j)
			bv[j] = *reinterpret_cast<const i32x4_t *>(I + b_row + j * 32 * 128);
	};
	auto mfma_block = [&](const i32x4_t (&av)[S::AI], const i32x4_t (&bv)[2]) { // dependent MFMAs are four (two) issues apart
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[i], bv[j], acc[i][j], 0, 0, 0);
	};

	load_step(0);
	store_step(0);
	if (steps > 1)
		load_step(1);
	lds_barrier();
	for (uint32_t k = 0; k < steps; ++k) {
		const int buf = (int)(k & 1u);
		i32x4_t av0[S::AI], bv0[2], av1[S::AI], bv1[2];
		read_block(buf, 0, av0, bv0);
		if (k + 1 < steps)
			store_step(buf ^ 1); // step k + 1, loaded a whole step ago; the idle buffer's readers passed the last barrier
		read_block(buf, 1, av1, bv1);
		if (k + 2 < steps)
			load_step(k + 2); // lands during the next step's MFMAs
		mfma_block(av0, bv0);
		read_block(buf, 2, av0, bv0);
		mfma_block(av1, bv1);
		read_block(buf, 3, av1, bv1);
		mfma_block(av0, bv0);
		mfma_block(av1, bv1);
		lds_barrier();
	}
}

// The range epilogue with the pair test of exact_range_codes.h in the place of !(score > theta):
// C[row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][col = lane & 31]; a lane holds its two columns' {sx, errx, Nx, m} and reads a
// query's {sqm, c1, c2, c3} as one 16-byte LDS word (two addresses per wave).  A surviving pair's 16-bit code (query in tile
// << LOG_W | row in tile) goes into the dead operand images — a wave reserves room by ballot with one LDS atomic — and the
// workgroup appends the n pairs to the launch's candidate buffer with ONE global atomic: k_range_candidates' compaction.
// n_q: the tile's queries that exist; pair(code): the (query, slot) a code stands for.
template <int QH, class Pair>
__device__ __forceinline__ void range_i8_keep(unsigned char *smem, const i32x16_t (&acc)[RangeI8Shape<QH>::AI][2],
                                              const RangeCodesRow (&col)[2], const bool (&col_live)[2], const RangeCodesQuery *qc_l,
                                              uint32_t n_q, uint32_t *n_staged, uint32_t *g_base, uint32_t *cand_count, uint2 *cand,
                                              Pair pair) {
	using S = RangeI8Shape<QH>;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = tid >> 6;
	const int wm = wave / S::WN, wn = wave % S::WN;
	uint16_t *staged = reinterpret_cast<uint16_t *>(smem); // QH x W codes at the most: 32 or 16 KiB
#pragma unroll
	for (int i = 0; i < S::AI; ++i) {
#pragma unroll
		for (int e = 0; e < 16; ++e) {
			const uint32_t ql = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * ((uint32_t)lane >> 5);
			const RangeCodesQuery q = qc_l[ql];
#pragma unroll
			for (int j = 0; j < 2; ++j) {
				const uint32_t cl = wn * 64 + j * 32 + (lane & 31);
				const bool keep = col_live[j] && ql < n_q && range_codes_keep(acc[i][j][e], q, col[j]);
				const unsigned long long m = __ballot(keep);
				if (m) { // (wave-uniform)
					uint32_t base = 0;
					if (lane == 0)
						base = atomicAdd(n_staged, (uint32_t)__popcll(m));
					base = __shfl(base, 0);
					if (keep)
						staged[base + __popcll(m & lanes_below(lane))] = (uint16_t)(ql << S::LOG_W | cl);
				}
			}
		}
	}
	__syncthreads();
	const uint32_t n = *n_staged;
	if (n == 0)
		return;
	if (tid == 0)
		*g_base = atomicAdd(cand_count, n);
	__syncthreads();
	uint2 *out = cand + *g_base;
	for (uint32_t t = tid; t < n; t += 256)
		out[t] = pair(staged[t]);
}

// a query of the tile that does not exist: every finite W is dropped (and `ql < n_q` refuses the rest)
__device__ __forceinline__ RangeCodesQuery range_i8_no_query() {
	return RangeCodesQuery {0.f, 0.f, 0.f, __builtin_inff()};
}

// ---------------------------------------------------------------------------------------------------------
// The dense tile: queries q0 .. and rows r0 .. of the launch, clamped at its edges; padding never survives, nor does a removed row.
template <int MT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_range_candidates_i8(RangeTileArgs a, RangeCodesView v) {
	using S = RangeI8Shape<128>;
	extern __shared__ __attribute__((aligned(16))) unsigned char ri_smem[];
	__shared__ __attribute__((aligned(16))) RangeCodesQuery qc_l[128];
	__shared__ uint32_t n_staged, g_base;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wn = (tid >> 6) % S::WN;
	const uint32_t q0 = a.q_begin + blockIdx.y * 128u, r0 = a.row_begin + blockIdx.x * 128u;
	if (tid < 128)
		qc_l[tid] = q0 + tid < a.q_end ? v.qc[q0 + tid] : range_i8_no_query();
	if (tid == 0)
		n_staged = 0u;
	const uint32_t rr = (uint32_t)tid >> 3;
	RangeI8Sources<128> src;
#pragma unroll
	for (int p = 0; p < 4; ++p) {
		uint32_t qi = q0 + rr + 32u * p, ri = r0 + rr + 32u * p;
		qi = qi < a.q_end ? qi : a.q_end - 1u;
		ri = ri < a.row_end ? ri : a.row_end - 1u;
		src.q[p] = reinterpret_cast<const i32x4_t *>(v.q_codes + (size_t)qi * a.V);
		src.x[p] = reinterpret_cast<const i32x4_t *>(v.row_codes + (size_t)ri * a.V);
	}
	// what the epilogue reads from memory, asked for ahead of the loop: the records of this lane's two columns
	RangeCodesRow col[2];
	bool col_live[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t c = r0 + wn * 64 + j * 32 + (lane & 31), cc = c < a.row_end ? c : a.row_end - 1u;
		col[j] = range_codes_row(MT, a.V * 4u, v.row_meta[cc]);
		col_live[j] = c < a.row_end && a.keys[cc] != FREE_KEY;
	}
	i32x16_t acc[2][2];
	range_i8_dots<128>(ri_smem, src, a.V / 4u, acc); // (V % 8 == 0: the host's choice of this kernel)
	range_i8_keep<128>(ri_smem, acc, col, col_live, qc_l, a.q_end - q0, &n_staged, &g_base, a.cand_count, a.cand,
	                   [&](uint32_t code) { return make_uint2(q0 + (code >> 7), r0 + (code & 127u)); });
}

// The gathered tile: row r of the B operand = the code row of slot lists[list_offset + pos], query t of the A operand = the
// codes of query order[first_query + t].  List entries and the columns' records — read through the list as well — are fetched
// ahead of the K loop.  Listed rows are live; positions from the end of the list or of the launch's run, and queries from
// n_queries, are padding.
template <int MT, int QH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_range_candidates_lists_i8(RangeListTileArgs a,
                                                                                                         RangeCodesView v) {
	using S = RangeI8Shape<QH>;
	extern __shared__ __attribute__((aligned(16))) unsigned char ri_smem[];
	__shared__ __attribute__((aligned(16))) RangeCodesQuery qc_l[QH];
	__shared__ uint32_t n_staged, g_base;
	const host::ExactFilterTile tile = a.tiles[a.tile_index[blockIdx.y]];
	const uint32_t end = tile.list_length < a.pos_end ? tile.list_length : a.pos_end; // of this tile's positions in the launch
	const uint32_t p0 = a.pos_begin + blockIdx.x * S::W;
	if (p0 >= end) // (uniform over the workgroup) the grid follows the launch's longest list
		return;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wn = (tid >> 6) % S::WN;
	const uint32_t *order = a.order + tile.first_query, *list = a.lists + tile.list_offset;
	if (tid < QH)
		qc_l[tid] = (uint32_t)tid < tile.n_queries ? v.qc[order[tid]] : range_i8_no_query();
	if (tid == 0)
		n_staged = 0u;
	const uint32_t rr = (uint32_t)tid >> 3;
	RangeI8Sources<QH> src;
#pragma unroll
	for (int p = 0; p < S::PA; ++p) {
		const uint32_t t = rr + 32u * p;
		src.q[p] = reinterpret_cast<const i32x4_t *>(v.q_codes + (size_t)order[t < tile.n_queries ? t : tile.n_queries - 1u] * a.V);
	}
#pragma unroll
	for (int p = 0; p < S::PB; ++p) {
		const uint32_t pos = p0 + rr + 32u * p;
		src.x[p] = reinterpret_cast<const i32x4_t *>(v.row_codes + (size_t)list[pos < end ? pos : end - 1u] * a.V);
	}
	RangeCodesRow col[2];
	bool col_live[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t c = p0 + wn * 64 + j * 32 + (lane & 31);
		col[j] = range_codes_row(MT, a.V * 4u, v.row_meta[list[c < end ? c : end - 1u]]);
		col_live[j] = c < end;
	}
	i32x16_t acc[S::AI][2];
	range_i8_dots<QH>(ri_smem, src, a.V / 4u, acc);
	range_i8_keep<QH>(ri_smem, acc, col, col_live, qc_l, tile.n_queries, &n_staged, &g_base, a.cand_count, a.cand,
	                  [&](uint32_t code) { return make_uint2(order[code >> S::LOG_W], list[p0 + (code & (S::W - 1u))]); });
}

// ---------------------------------------------------------------------------------------------------------
hipError_t launch_range_prepare_codes(const RangeCodesPrepareArgs &a, hipStream_t stream) {
	hipLaunchKernelGGL(k_range_prepare_codes, dim3((a.n_queries + 255u) / 256u), dim3(256), 0, stream, a);
	return hipGetLastError();
}

template <int MT>
static hipError_t launch_range_candidates_i8_as(const RangeTileArgs &a, const RangeCodesView &c, hipStream_t stream) {
	constexpr uint32_t lds = RangeI8Shape<128>::LDS_BYTES;
	if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_range_candidates_i8<MT>),
	                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
		return e;
	const dim3 grid((a.row_end - a.row_begin + 127u) / 128u, (a.q_end - a.q_begin + 127u) / 128u);
	hipLaunchKernelGGL(k_range_candidates_i8<MT>, grid, dim3(256), lds, stream, a, c);
	return hipGetLastError();
}

hipError_t launch_range_candidates_i8(const RangeTileArgs &a, const RangeCodesView &c, hipStream_t stream) {
	return a.metric == 0   ? launch_range_candidates_i8_as<0>(a, c, stream)
	       : a.metric == 1 ? launch_range_candidates_i8_as<1>(a, c, stream)
	                       : launch_range_candidates_i8_as<2>(a, c, stream);
}

template <int MT, int QH>
static hipError_t launch_range_candidates_lists_i8_as(const RangeListTileArgs &a, const RangeCodesView &c, hipStream_t stream) {
	using S = RangeI8Shape<QH>;
	if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_range_candidates_lists_i8<MT, QH>),
	                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::LDS_BYTES))
		return e;
	const dim3 grid((a.pos_end - a.pos_begin + S::W - 1u) / S::W, a.n_tiles);
	hipLaunchKernelGGL((k_range_candidates_lists_i8<MT, QH>), grid, dim3(256), S::LDS_BYTES, stream, a, c);
	return hipGetLastError();
}

hipError_t launch_range_candidates_lists_i8(const RangeListTileArgs &a, bool small, const RangeCodesView &c, hipStream_t stream) {
	if (!a.n_tiles || a.pos_begin >= a.pos_end)
		return hipSuccess;
	if (small)
		return a.metric == 0   ? launch_range_candidates_lists_i8_as<0, 32>(a, c, stream)
		       : a.metric == 1 ? launch_range_candidates_lists_i8_as<1, 32>(a, c, stream)
		                       : launch_range_candidates_lists_i8_as<2, 32>(a, c, stream);
	return a.metric == 0   ? launch_range_candidates_lists_i8_as<0, 128>(a, c, stream)
	       : a.metric == 1 ? launch_range_candidates_lists_i8_as<1, 128>(a, c, stream)
	                       : launch_range_candidates_lists_i8_as<2, 128>(a, c, stream);
}

#endif // VSS_EXACT_RANGE_CODES_TU

} // namespace vss
