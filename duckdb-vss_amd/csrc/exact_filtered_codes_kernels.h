// exact_filtered_codes_kernels.h — the filtered exact search's BOUND tile on the int8 matrix pipe, over the index's resident
// 8-bit row codes gathered through the predicates' lists (option exact.filtered_codes_i8, score kind 2).
//
//   k_exact_filtered_bounds_i8   pass A of the filtered exact search by bounds: where k_exact_filtered_scores writes a pair's
//                                metric distance, this tile writes U(I), the upper bound of exact_codes_bound.h from the integer
//                                dot product of the two codes — the same cell of `scores`, so the unchanged k_exact_select_lists
//                                leaves best_s[t][k - 1] = tau, the k-th smallest upper bound of position t's list
//
// Pass B is the gathered int8 range tile (k_range_candidates_lists_i8) under the radii tau with the range re-score, and
// k_exact_codes_topk takes the k smallest (distance, slot) of the matches: exact_codes_kernels.h has the argument.
//
// The engine includes this header for the launcher; the kernel is defined once, in exact_filtered_codes.hip.
#pragma once
#include "exact_range_kernels.h"

namespace vss {

// one (pass, chunk) of pass A in one of the two shapes: workgroup row y takes tile tiles[tile_index[y]], its workgroups stride
// over the blocks of list positions [pos_begin, pos_begin + chunk_stride) that the tile's list has
struct FilteredBoundArgs {
	const uint32_t *order; // the group order: position -> original query index
	const uint32_t *lists; // the pass's lists of live admitted slots
	const host::ExactFilterTile *tiles;
	const uint32_t *tile_index;
	uint32_t n_tiles;
	uint32_t V;
	uint32_t pos_begin, chunk_stride;
	int metric;
	float *scores; // [position of the group order][chunk_stride]: k_exact_filtered_scores' cells
};

// small: the 32-query shape.  blocks_x: workgroups per tile (each strides over its tile's blocks).  c.q_codes and c.qc are read
// by ORIGINAL query index.  Needs V % 8 == 0.
hipError_t launch_exact_filtered_bounds_i8(const FilteredBoundArgs &a, bool small, const ExactCodesView &c, uint32_t blocks_x,
                                           hipStream_t stream);

#ifdef VSS_EXACT_FILTERED_CODES_TU

typedef int xf_i32x16 __attribute__((ext_vector_type(16)));
typedef int xf_i32x4 __attribute__((ext_vector_type(4)));

// QH queries x W list positions per block, 256 threads: the gathered int8 range tile's two shapes
//   QH = 128  2 x 2 waves of 64 x 64 (2 x 2 accumulators of sixteen i32): 128 x 128
//   QH = 32   four waves side by side along the positions, 32 x 64 each (1 x 2 accumulators): 32 x 256
template <int QH>
struct FilteredBoundShape {
	static constexpr uint32_t W = QH == 128 ? 128 : 256;
	static constexpr int WN = W / 64;               // waves along the positions (4 / WN along the queries)
	static constexpr int AI = QH == 128 ? 2 : 1;    // accumulators of a wave along the queries (two along the positions)
	static constexpr int PA = QH / 32, PB = W / 32; // chunks a loading thread stages per step and operand
	static constexpr uint32_t A_BYTES = QH * 128, BUF_BYTES = (QH + W) * 128, LDS_BYTES = 2 * BUF_BYTES;
};

// The tile.  A workgroup keeps ONE tile of the plan — its queries, their code rows' addresses and their bound constants are
// set up once — and strides over that tile's blocks of W list positions; everything that depends on the block is asked for a
// block ahead, so that the K loop never waits for a list entry:
//   * operands travel as in k_exact_bounds_i8: a K step is 128 code bytes = four MFMA blocks of depth 32; an operand image is
//     rows x 128 bytes, chunk c (16 bytes) of row r at position c ^ (r & 7) (conflict-free on both sides: the range tile's comment
//     has the argument); two buffers, ONE LDS-only barrier per step; the registers loaded during step g - 1 are written to the
//     idle buffer at the top of step g and the loads of step g + 2 go out behind them.  The load cursor runs two steps ahead of
//     the MFMAs through ALL the workgroup's blocks: a gathered row of 128 dimensions is a single step, and a per-block prologue
//     would be the whole of it;
//   * the B operand's rows are slots read through the list.  The entries of block b + 1 of the workgroup are loaded when the load
//     cursor enters block b (`ahead`), a block's worth of steps before their code rows are addressed; the entries of the two
//     columns a lane finishes in the epilogue are loaded in the last step of the block before (`col_next`), their code records
//     in the block's own last step, under its MFMAs;
//   * positions beyond the end of the list or of the chunk re-read the last one (the load) and are never written (the epilogue);
//     queries beyond the tile's re-read its last one; a chunk beyond a row's V / 4 is staged as zeros.
// Epilogue: C[query = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][position = lane & 31]; a query's {sqm, c1, c2, c3} is one 16-byte LDS
// word; U = exact_codes_upper, and a half-wave's 32 positions of one query are one 128-byte line of `scores`.
template <int MT, int QH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_exact_filtered_bounds_i8(FilteredBoundArgs a,
                                                                                                        ExactCodesView v) {
	using S = FilteredBoundShape<QH>;
	extern __shared__ __attribute__((aligned(16))) unsigned char xf_smem[];
	__shared__ __attribute__((aligned(16))) ExactCodesQuery qc_l[QH];
	const host::ExactFilterTile tile = a.tiles[a.tile_index[blockIdx.y]];
	if (tile.list_length <= a.pos_begin) // (uniform over the workgroup) this list ended in an earlier chunk
		return;
	// everything below is RELATIVE to pos_begin: n_rel <= chunk_stride, so no position arithmetic can pass 2^32
	const uint32_t n_rel = tile.list_length - a.pos_begin < a.chunk_stride ? tile.list_length - a.pos_begin : a.chunk_stride;
	const uint32_t n_blocks = (n_rel + S::W - 1u) / S::W, G = gridDim.x, b0 = blockIdx.x;
	if (b0 >= n_blocks)
		return;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int wm = wave / S::WN, wn = wave % S::WN;
	const uint32_t chunks = a.V / 4u, steps = (chunks + 7u) / 8u; // (V % 8 == 0: the host's choice of this kernel)
	const uint32_t N = ((n_blocks - b0 + G - 1u) / G) * steps;    // steps of this workgroup, all its blocks in a row
	const uint32_t *order = a.order + tile.first_query, *list = a.lists + tile.list_offset + a.pos_begin;
	if (tid < QH)
		qc_l[tid] = v.qc[order[(uint32_t)tid < tile.n_queries ? (uint32_t)tid : tile.n_queries - 1u]];

	xf_i32x16 acc[S::AI][2];
#pragma unroll
	for (int i = 0; i < S::AI; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[i][j][e] = 0;

	// ---- the load side: thread -> chunk f of the step's eight, rows rr + 32 p of both operands
	const uint32_t f = (uint32_t)tid & 7u, rr = (uint32_t)tid >> 3;
	const uint32_t st_off = rr * 128u + ((f ^ (rr & 7u)) << 4); // (rows rr + 32 p: the same row & 7)
	const xf_i32x4 *q_src[S::PA], *x_src[S::PB];
#pragma unroll
	for (int p = 0; p < S::PA; ++p) {
		const uint32_t t = rr + 32u * p;
		q_src[p] = reinterpret_cast<const xf_i32x4 *>(v.q_codes + (size_t)order[t < tile.n_queries ? t : tile.n_queries - 1u] * a.V);
	}
	auto entry = [&](uint32_t rel) { return list[rel < n_rel ? rel : n_rel - 1u]; }; // the slot at a relative position, clamped
	uint32_t ahead[S::PB]; // the slots of the block the load cursor enters NEXT
	auto ask_ahead = [&](uint32_t block) {
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			ahead[p] = entry(block * S::W + rr + 32u * p);
	};
	uint32_t block_l = b0, step_l = 0; // the load cursor: two steps ahead of the MFMAs, possibly in the next block already
	auto enter_block = [&]() {        // `ahead` holds block_l's slots
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			x_src[p] = reinterpret_cast<const xf_i32x4 *>(v.row_codes + (size_t)ahead[p] * a.V);
		if (block_l + G < n_blocks)
			ask_ahead(block_l + G);
	};
	xf_i32x4 qa[S::PA], xb[S::PB];
	auto load_next = [&]() { // the step under the load cursor -> registers (clamped chunk, zeroed afterwards); advances the cursor
		const uint32_t c = step_l * 8u + f, cc = c < chunks ? c : chunks - 1u;
#pragma unroll
		for (int p = 0; p < S::PA; ++p)
			qa[p] = q_src[p][cc];
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			xb[p] = x_src[p][cc];
		if (c >= chunks) {
#pragma unroll
			for (int p = 0; p < S::PA; ++p)
				qa[p] = xf_i32x4 {0, 0, 0, 0};
#pragma unroll
			for (int p = 0; p < S::PB; ++p)
				xb[p] = xf_i32x4 {0, 0, 0, 0};
		}
		if (++step_l == steps) {
			step_l = 0;
			block_l += G;
			if (block_l < n_blocks)
				enter_block();
		}
	};
	auto store_step = [&](int buf) {
		unsigned char *A = xf_smem + buf * S::BUF_BYTES + st_off, *B = A + S::A_BYTES;
#pragma unroll
		for (int p = 0; p < S::PA; ++p)
			*reinterpret_cast<xf_i32x4 *>(A + p * 32 * 128) = qa[p];
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			*reinterpret_cast<xf_i32x4 *>(B + p * 32 * 128) = xb[p];
	};
	// ---- the MFMA side: row lane & 31 of each 32-row tile, chunk 2 kb + (lane >> 5) of block kb, at its swizzled position
	const uint32_t a_row = (uint32_t)(wm * 64 + (lane & 31)) * 128u, b_row = S::A_BYTES + (uint32_t)(wn * 64 + (lane & 31)) * 128u;
	uint32_t pos[4];
#pragma unroll
	for (int kb = 0; kb < 4; ++kb)
		pos[kb] = (((uint32_t)(2 * kb) + ((uint32_t)lane >> 5)) ^ ((uint32_t)lane & 7u)) << 4;
	auto read_block = [&](int buf, int kb, xf_i32x4 (&av)[S::AI], xf_i32x4 (&bv)[2]) {
		const unsigned char *I = xf_smem + buf * S::BUF_BYTES + pos[kb];
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
			av[i] = *reinterpret_cast<const xf_i32x4 *>(I + a_row + i * 32 * 128);
#pragma unroll
		for (int j = 0; j < 2; ++j)
			bv[j] = *reinterpret_cast<const xf_i32x4 *>(I + b_row + j * 32 * 128);
	};
	auto mfma_block = [&](const xf_i32x4 (&av)[S::AI], const xf_i32x4 (&bv)[2]) { // dependent MFMAs are four (two) issues apart
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[i], bv[j], acc[i][j], 0, 0, 0);
	};

	// prologue: the first block's slots, this workgroup's first step into buffer 0, the second on its way
	const uint32_t col_off = (uint32_t)(wn * 64 + (lane & 31)); // this lane's first column of a block; the second is 32 on
	uint32_t col_next[2] = {entry(b0 * S::W + col_off), entry(b0 * S::W + col_off + 32u)};
	ask_ahead(b0);
	enter_block();
	load_next();
	store_step(0);
	if (N > 1)
		load_next();
	lds_barrier(); // (qc_l is in place behind it too)
	uint32_t block_c = b0, step_c = 0; // the compute cursor
	RowCodeMeta col_meta[2];
#pragma unroll
	for (int j = 0; j < 2; ++j)
		col_meta[j] = RowCodeMeta {0.f, 0.f, 0.f, 0};
	for (uint32_t g = 0; g < N; ++g) {
		const int buf = (int)(g & 1u);
		const bool last = step_c + 1 == steps;
		if (last) { // what the epilogue reads from memory, under the step's MFMAs; the next block's columns behind it
#pragma unroll
			for (int j = 0; j < 2; ++j)
				col_meta[j] = v.row_meta[col_next[j]];
			if (block_c + G < n_blocks) {
#pragma unroll
				for (int j = 0; j < 2; ++j)
					col_next[j] = entry((block_c + G) * S::W + col_off + 32u * j);
			}
		}
		xf_i32x4 av0[S::AI], bv0[2], av1[S::AI], bv1[2];
		read_block(buf, 0, av0, bv0);
		if (g + 1 < N)
			store_step(buf ^ 1); // step g + 1, loaded a whole step ago; the idle buffer's readers passed the last barrier
		read_block(buf, 1, av1, bv1);
		if (g + 2 < N)
			load_next(); // lands during the next step's MFMAs
		mfma_block(av0, bv0);
		read_block(buf, 2, av0, bv0);
		mfma_block(av1, bv1);
		read_block(buf, 3, av1, bv1);
		mfma_block(av0, bv0);
		mfma_block(av1, bv1);
		lds_barrier();
		if (!last) {
			++step_c;
			continue;
		}
		// ---- epilogue of block block_c: registers and qc_l only, so the other waves go on into the next block's steps
#pragma unroll
		for (int j = 0; j < 2; ++j) {
			const uint32_t rel = block_c * S::W + col_off + 32u * j;
			if (rel >= n_rel)
				continue;
			const ExactCodesRow row = exact_codes_row(MT, a.V * 4u, col_meta[j]);
			float *out = a.scores + (size_t)tile.first_query * a.chunk_stride + rel;
#pragma unroll
			for (int i = 0; i < S::AI; ++i) {
#pragma unroll
				for (int e = 0; e < 16; ++e) {
					const uint32_t ql = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * ((uint32_t)lane >> 5);
					if (ql < tile.n_queries)
						out[(size_t)ql * a.chunk_stride] = exact_codes_upper(acc[i][j][e], qc_l[ql], row);
				}
			}
		}
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
#pragma unroll
				for (int e = 0; e < 16; ++e)
					acc[i][j][e] = 0;
		block_c += G;
		step_c = 0;
	}
}

// ---------------------------------------------------------------------------------------------------------
template <int MT, int QH>
static hipError_t launch_exact_filtered_bounds_i8_as(const FilteredBoundArgs &a, const ExactCodesView &c, uint32_t blocks_x,
                                                     hipStream_t stream) {
	using S = FilteredBoundShape<QH>;
	if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_exact_filtered_bounds_i8<MT, QH>),
	                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::LDS_BYTES))
		return e;
	const uint32_t most = (a.chunk_stride + S::W - 1u) / S::W; // blocks of the longest possible list run
	const dim3 grid(blocks_x < most ? (blocks_x ? blocks_x : 1u) : most, a.n_tiles);
	hipLaunchKernelGGL((k_exact_filtered_bounds_i8<MT, QH>), grid, dim3(256), S::LDS_BYTES, stream, a, c);
	return hipGetLastError();
}

hipError_t launch_exact_filtered_bounds_i8(const FilteredBoundArgs &a, bool small, const ExactCodesView &c, uint32_t blocks_x,
                                           hipStream_t stream) {
	if (!a.n_tiles || !a.chunk_stride)
		return hipSuccess;
	if (small)
		return a.metric == 0   ? launch_exact_filtered_bounds_i8_as<0, 32>(a, c, blocks_x, stream)
		       : a.metric == 1 ? launch_exact_filtered_bounds_i8_as<1, 32>(a, c, blocks_x, stream)
		                       : launch_exact_filtered_bounds_i8_as<2, 32>(a, c, blocks_x, stream);
	return a.metric == 0   ? launch_exact_filtered_bounds_i8_as<0, 128>(a, c, blocks_x, stream)
	       : a.metric == 1 ? launch_exact_filtered_bounds_i8_as<1, 128>(a, c, blocks_x, stream)
	                       : launch_exact_filtered_bounds_i8_as<2, 128>(a, c, blocks_x, stream);
}

#endif // VSS_EXACT_FILTERED_CODES_TU

} // namespace vss
