// exact_range_split_kernels.h — the range search's candidate tiles on the bf16 matrix pipe (option range.split_bf16).
//
//   k_range_candidates_bf16x3         k_range_candidates' 128 queries x 128 rows with  q.x ~ sum qh xh + qh xl + ql xh  on
//                                     v_mfma_f32_32x32x16_bf16: three MFMAs of depth 16 where the f32 tile issues eight of depth 2
//   k_range_candidates_lists_bf16x3   the same for k_range_candidates_lists, in its two shapes (128 x 128 and 32 x 256)
//
// The score only PROPOSES pairs.  The threshold they are held against (k_range_prepare, score kind 1) carries the error bound of
// this sum, exact_cert_error_split, so no matching pair is dropped; a wider bound hands a few more pairs to the re-score in the
// metric, which decides.  Nothing is certified afterwards and nothing redone: the answers are those of the f32 tiles.
//
// Included at the end of exact_range_kernels.h; the kernels are defined once, in exact_range.hip, which is built without packed
// f32 arithmetic as the split needs (the remainders x - hi are single v_sub_f32).  split_pair, split_chunk and xs_swizzle are
// exact_split_kernels.h's, the queries arrive split by its launch_split_queries.
#pragma once

namespace vss {

// q_hi / q_lo: the padded query block as launch_split_queries writes it — V / 2 cells of eight bf16 per query in each array, by
// ORIGINAL query index.  Both need V % 8 == 0 (whole steps of 32 floats).
hipError_t launch_range_candidates_bf16x3(const RangeTileArgs &a, const uint4 *q_hi, const uint4 *q_lo, hipStream_t stream);
hipError_t launch_range_candidates_lists_bf16x3(const RangeListTileArgs &a, bool small, const uint4 *q_hi, const uint4 *q_lo,
                                                hipStream_t stream); // small: the 32-query shape

#ifdef VSS_EXACT_RANGE_TU

// ---------------------------------------------------------------------------------------------------------
// One workgroup's tile: QH queries x W rows, 256 threads.
//   QH = 128  2 x 2 waves of 64 x 64 (2 x 2 accumulators): 128 x 128, the dense tile and the gathered tile's tall shape
//   QH = 32   four waves side by side along the rows, 32 x 64 each (1 x 2 accumulators): 32 x 256, the gathered tile's other shape
// Operand staging, K step 32 floats = two MFMA blocks of depth 16:
//   * per operand a hi image and a lo image of bf16, a row = 64 bytes = four chunks of eight bf16, chunk c of row r at position
//     c ^ xs_swizzle(r): the staging write (four chunks of consecutive rows) and the MFMA side's ds_read_b128 (32 consecutive
//     rows at one chunk) both spread over all banks.  A buffer is A hi | A lo | B hi | B lo = (QH + W) x 128 bytes, what the f32
//     tile's buffer is; two buffers: 64 KiB, or 72 KiB for the 32-query shape, so two workgroups fit a compute unit;
//   * rows are split on the way in: thread -> chunk tid & 3 of rows tid >> 2 + 64 p, two global_load_dwordx4 per row, issued
//     two steps ahead, converted (split_chunk) and written to the idle buffer one step ahead;
//   * queries arrive split: one 16-byte load per image and row, written as it is (the 32-query shape: by 128 threads);
//   * ONE barrier per step, an LDS-only one, so the global loads stay in flight across it;
//   * per block of depth 16 and accumulator hi.hi, hi.lo, lo.hi, in this order, term-major over the accumulators so that
//     dependent MFMAs are four (two) issues apart.  A lane supplies row lane & 31 and the eight k of chunk 2 kb + (lane >> 5)
//     on both operands alike.
template <int QH>
struct RangeSplitShape {
	static constexpr uint32_t W = QH == 128 ? 128 : 256, LOG_W = QH == 128 ? 7 : 8; // rows per workgroup
	static constexpr int WN = W / 64;                                                // waves along the rows (4 / WN along the queries)
	static constexpr int AI = QH == 128 ? 2 : 1;                                     // accumulators of a wave along the queries (two along the rows)
	static constexpr int PA = QH == 128 ? 2 : 1, PB = W / 64;                        // rows a loading thread stages per step and operand
	static constexpr uint32_t A_IMAGE = QH * 64, B_IMAGE = W * 64;                   // one bf16 image of one operand and step
	static constexpr uint32_t BUF_BYTES = 2 * (A_IMAGE + B_IMAGE), LDS_BYTES = 2 * BUF_BYTES;
};

// what a loading thread reads: its chunk of its rows at step 0 (rows beyond the edge re-read the last one)
template <int QH>
struct RangeSplitSources {
	const u32x4_t *qh[RangeSplitShape<QH>::PA], *ql[RangeSplitShape<QH>::PA]; // + 4 per step
	const float4 *x[RangeSplitShape<QH>::PB];                                 // + 8 per step, two float4 each
};

// acc = the tile's dot products over `steps` steps.  Ends behind a barrier: the operand images are dead on return.
template <int QH>
__device__ __forceinline__ void range_split_dots(unsigned char *smem, const RangeSplitSources<QH> &src, uint32_t steps,
                                                 f32x16 (&acc)[RangeSplitShape<QH>::AI][2]) {
	using S = RangeSplitShape<QH>;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int wm = wave / S::WN, wn = wave % S::WN;
#pragma unroll
	for (int i = 0; i < S::AI; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[i][j][e] = 0.f;

	// ---- the load side
	const uint32_t c = (uint32_t)tid & 3u, rr = (uint32_t)tid >> 2;
	const uint32_t st_off = rr * 64u + ((c ^ xs_swizzle(rr)) * 16u); // (row + 64 has the same swizzle: + 64 * 64 bytes)
	const bool stages_a = QH == 128 || wave < 2;                    // (wave-uniform) 32 queries x 4 chunks = 128 threads
	u32x4_t qh[S::PA], ql[S::PA];
	float4 x0[S::PB], x1[S::PB]; // (the two halves of a row's 32 bytes)
#pragma unroll
	for (int p = 0; p < S::PA; ++p)
		qh[p] = ql[p] = u32x4_t {0u, 0u, 0u, 0u};
	auto load_step = [&](uint32_t step) {
		if (stages_a) {
#pragma unroll
			for (int p = 0; p < S::PA; ++p)
				qh[p] = src.qh[p][step * 4u], ql[p] = src.ql[p][step * 4u];
		}
#pragma unroll
		for (int p = 0; p < S::PB; ++p)
			x0[p] = src.x[p][step * 8u], x1[p] = src.x[p][step * 8u + 1u];
	};
	auto store_step = [&](int buf) { // the registers -> LDS buffer `buf`; the rows are split here, once per element and workgroup
		unsigned char *A = smem + buf * S::BUF_BYTES + st_off, *B = A + 2 * S::A_IMAGE;
		if (stages_a) {
#pragma unroll
			for (int p = 0; p < S::PA; ++p) {
				*reinterpret_cast<u32x4_t *>(A + p * 4096) = qh[p];
				*reinterpret_cast<u32x4_t *>(A + S::A_IMAGE + p * 4096) = ql[p];
			}
		}
#pragma unroll
		for (int p = 0; p < S::PB; ++p) {
			uint4 h, l;
			split_chunk(x0[p], x1[p], h, l);
			*reinterpret_cast<uint4 *>(B + p * 4096) = h;
			*reinterpret_cast<uint4 *>(B + S::B_IMAGE + p * 4096) = l;
		}
	};
	// ---- the MFMA side: row lane & 31 of each 32-row tile, chunk 2 kb + (lane >> 5) of block kb, at its swizzled position
	const uint32_t a_row = (uint32_t)(wm * 64 + (lane & 31)) * 64u, b_row = 2 * S::A_IMAGE + (uint32_t)(wn * 64 + (lane & 31)) * 64u;
	uint32_t pos[2];
#pragma unroll
	for (int kb = 0; kb < 2; ++kb)
		pos[kb] = (((uint32_t)(2 * kb) + ((uint32_t)lane >> 5)) ^ xs_swizzle((uint32_t)lane & 31u)) * 16u;
	struct Operands {
		uint4 ah[S::AI], al[S::AI], bh[2], bl[2];
	};
	auto read_block = [&](int buf, int kb, Operands &o) {
		const unsigned char *I = smem + buf * S::BUF_BYTES + pos[kb];
#pragma unroll
		for (int i = 0; i < S::AI; ++i) {
			o.ah[i] = *reinterpret_cast<const uint4 *>(I + a_row + i * 32 * 64);
			o.al[i] = *reinterpret_cast<const uint4 *>(I + S::A_IMAGE + a_row + i * 32 * 64);
		}
#pragma unroll
		for (int j = 0; j < 2; ++j) {
			o.bh[j] = *reinterpret_cast<const uint4 *>(I + b_row + j * 32 * 64);
			o.bl[j] = *reinterpret_cast<const uint4 *>(I + S::B_IMAGE + b_row + j * 32 * 64);
		}
	};
	auto mfma = [&](const uint4 &x, const uint4 &y, f32x16 &d) {
		d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, x), __builtin_bit_cast(bf16x8_t, y), d, 0, 0, 0);
	};
	auto mfma_block = [&](const Operands &o) { // hi.hi, hi.lo, lo.hi: the order is fixed
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				mfma(o.ah[i], o.bh[j], acc[i][j]);
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				mfma(o.ah[i], o.bl[j], acc[i][j]);
#pragma unroll
		for (int i = 0; i < S::AI; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				mfma(o.al[i], o.bh[j], acc[i][j]);
	};

	load_step(0);
	store_step(0);
	if (steps > 1)
		load_step(1);
	lds_barrier();
	for (uint32_t k = 0; k < steps; ++k) {
		const int buf = (int)(k & 1u);
		Operands o0, o1;
		read_block(buf, 0, o0);
		if (k + 1 < steps)
			store_step(buf ^ 1); // step k + 1, loaded a whole step ago; the idle buffer's readers passed the last barrier
		read_block(buf, 1, o1);
		if (k + 2 < steps)
			load_step(k + 2); // lands during the next step's MFMAs
		mfma_block(o0);
		mfma_block(o1);
		lds_barrier();
	}
}

// The range epilogue, k_range_candidates' own: C[row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][col = lane & 31]; a pair survives
// with !(score > theta), which keeps a NaN score; its 16-bit code (query in tile << LOG_W | row in tile) goes into the dead
// operand images — a wave reserves room by ballot with one LDS atomic — and the workgroup appends the n pairs to the launch's
// candidate buffer with ONE global atomic.  n_q: the tile's queries that exist; pair(code): the (query, slot) a code stands for.
template <int MT, int QH, class Pair>
__device__ __forceinline__ void range_split_keep(unsigned char *smem, const f32x16 (&acc)[RangeSplitShape<QH>::AI][2],
                                                 const float (&col_n2)[2], const bool (&col_live)[2], const float *theta_l,
                                                 uint32_t n_q, uint32_t *n_staged, uint32_t *g_base, uint32_t *cand_count, uint2 *cand,
                                                 Pair pair) {
	using S = RangeSplitShape<QH>;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = tid >> 6;
	const int wm = wave / S::WN, wn = wave % S::WN;
	uint16_t *staged = reinterpret_cast<uint16_t *>(smem); // QH x W codes at the most: 32 or 16 KiB
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
				const bool keep = col_live[j] && ql < n_q && !(s > theta_l[ql]);
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

// ---------------------------------------------------------------------------------------------------------
// The dense tile: queries q0 .. and rows r0 .. of the launch, clamped at its edges; padding never survives (theta = -inf,
// col_live = false), nor does a removed row.
template <int MT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void
k_range_candidates_bf16x3(RangeTileArgs a, const uint4 *q_hi, const uint4 *q_lo) {
	using S = RangeSplitShape<128>;
	extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
	__shared__ float theta_l[128];
	__shared__ uint32_t n_staged, g_base;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wn = (tid >> 6) % S::WN;
	const uint32_t q0 = a.q_begin + blockIdx.y * 128u, r0 = a.row_begin + blockIdx.x * 128u;
	if (tid < 128)
		theta_l[tid] = q0 + tid < a.q_end ? a.theta[q0 + tid] : -__builtin_inff();
	if (tid == 0)
		n_staged = 0u;
	const uint32_t c = (uint32_t)tid & 3u, rr = (uint32_t)tid >> 2;
	RangeSplitSources<128> src;
#pragma unroll
	for (int p = 0; p < 2; ++p) {
		uint32_t qi = q0 + rr + 64u * p, ri = r0 + rr + 64u * p;
		qi = qi < a.q_end ? qi : a.q_end - 1u;
		ri = ri < a.row_end ? ri : a.row_end - 1u;
		src.qh[p] = reinterpret_cast<const u32x4_t *>(q_hi) + (size_t)qi * (a.V / 2u) + c; // (a query is V / 2 chunks in each array)
		src.ql[p] = reinterpret_cast<const u32x4_t *>(q_lo) + (size_t)qi * (a.V / 2u) + c;
		src.x[p] = a.vectors + (size_t)ri * a.V + 2u * c;
	}
	// what the epilogue reads from memory, asked for ahead of the loop: this lane's two columns
	float col_n2[2];
	bool col_live[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t col = r0 + wn * 64 + j * 32 + (lane & 31), cc = col < a.row_end ? col : a.row_end - 1u;
		col_n2[j] = a.row_norm2[cc];
		col_live[j] = col < a.row_end && a.keys[cc] != FREE_KEY;
	}
	f32x16 acc[2][2];
	range_split_dots<128>(rs_smem, src, a.V / 8u, acc); // (V % 8 == 0: the host's choice of this kernel)
	range_split_keep<MT, 128>(rs_smem, acc, col_n2, col_live, theta_l, a.q_end - q0, &n_staged, &g_base, a.cand_count, a.cand,
	                          [&](uint32_t code) { return make_uint2(q0 + (code >> 7), r0 + (code & 127u)); });
}

// The gathered tile: row r of the B operand = row lists[list_offset + pos] of the index, query t of the A operand = query
// order[first_query + t] of the pre-split arrays.  List entries and the columns' |x|^2 are fetched ahead of the K loop.  Listed
// rows are live; positions from the end of the list or of the launch's run, and queries from n_queries, are padding.
template <int MT, int QH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void
k_range_candidates_lists_bf16x3(RangeListTileArgs a, const uint4 *q_hi, const uint4 *q_lo) {
	using S = RangeSplitShape<QH>;
	extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
	__shared__ float theta_l[QH];
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
		theta_l[tid] = (uint32_t)tid < tile.n_queries ? a.theta[order[tid]] : -__builtin_inff();
	if (tid == 0)
		n_staged = 0u;
	const uint32_t c = (uint32_t)tid & 3u, rr = (uint32_t)tid >> 2;
	RangeSplitSources<QH> src;
#pragma unroll
	for (int p = 0; p < S::PA; ++p) {
		const uint32_t t = (QH == 128 ? rr : rr & 31u) + 64u * p; // (the 32-query shape: threads 128 .. stage no query)
		const size_t qi = order[t < tile.n_queries ? t : tile.n_queries - 1u];
		src.qh[p] = reinterpret_cast<const u32x4_t *>(q_hi) + qi * (a.V / 2u) + c;
		src.ql[p] = reinterpret_cast<const u32x4_t *>(q_lo) + qi * (a.V / 2u) + c;
	}
#pragma unroll
	for (int p = 0; p < S::PB; ++p) {
		const uint32_t pos = p0 + rr + 64u * p;
		src.x[p] = a.vectors + (size_t)list[pos < end ? pos : end - 1u] * a.V + 2u * c;
	}
	float col_n2[2];
	bool col_live[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const uint32_t col = p0 + wn * 64 + j * 32 + (lane & 31);
		col_n2[j] = a.row_norm2[list[col < end ? col : end - 1u]];
		col_live[j] = col < end;
	}
	f32x16 acc[S::AI][2];
	range_split_dots<QH>(rs_smem, src, a.V / 8u, acc);
	range_split_keep<MT, QH>(rs_smem, acc, col_n2, col_live, theta_l, tile.n_queries, &n_staged, &g_base, a.cand_count, a.cand,
	                         [&](uint32_t code) { return make_uint2(order[code >> S::LOG_W], list[p0 + (code & (S::W - 1u))]); });
}

// ---------------------------------------------------------------------------------------------------------
template <int MT>
static hipError_t launch_range_candidates_bf16x3_as(const RangeTileArgs &a, const uint4 *q_hi, const uint4 *q_lo, hipStream_t stream) {
	constexpr uint32_t lds = RangeSplitShape<128>::LDS_BYTES;
	if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_range_candidates_bf16x3<MT>),
	                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
		return e;
	const dim3 grid((a.row_end - a.row_begin + 127u) / 128u, (a.q_end - a.q_begin + 127u) / 128u);
	hipLaunchKernelGGL(k_range_candidates_bf16x3<MT>, grid, dim3(256), lds, stream, a, q_hi, q_lo);
	return hipGetLastError();
}

hipError_t launch_range_candidates_bf16x3(const RangeTileArgs &a, const uint4 *q_hi, const uint4 *q_lo, hipStream_t stream) {
	return a.metric == 0   ? launch_range_candidates_bf16x3_as<0>(a, q_hi, q_lo, stream)
	       : a.metric == 1 ? launch_range_candidates_bf16x3_as<1>(a, q_hi, q_lo, stream)
	                       : launch_range_candidates_bf16x3_as<2>(a, q_hi, q_lo, stream);
}

template <int MT, int QH>
static hipError_t launch_range_candidates_lists_bf16x3_as(const RangeListTileArgs &a, const uint4 *q_hi, const uint4 *q_lo,
                                                          hipStream_t stream) {
	using S = RangeSplitShape<QH>;
	if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_range_candidates_lists_bf16x3<MT, QH>),
	                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::LDS_BYTES))
		return e;
	const dim3 grid((a.pos_end - a.pos_begin + S::W - 1u) / S::W, a.n_tiles);
	hipLaunchKernelGGL((k_range_candidates_lists_bf16x3<MT, QH>), grid, dim3(256), S::LDS_BYTES, stream, a, q_hi, q_lo);
	return hipGetLastError();
}

hipError_t launch_range_candidates_lists_bf16x3(const RangeListTileArgs &a, bool small, const uint4 *q_hi, const uint4 *q_lo,
                                                hipStream_t stream) {
	if (!a.n_tiles || a.pos_begin >= a.pos_end)
		return hipSuccess;
	if (small)
		return a.metric == 0   ? launch_range_candidates_lists_bf16x3_as<0, 32>(a, q_hi, q_lo, stream)
		       : a.metric == 1 ? launch_range_candidates_lists_bf16x3_as<1, 32>(a, q_hi, q_lo, stream)
		                       : launch_range_candidates_lists_bf16x3_as<2, 32>(a, q_hi, q_lo, stream);
	return a.metric == 0   ? launch_range_candidates_lists_bf16x3_as<0, 128>(a, q_hi, q_lo, stream)
	       : a.metric == 1 ? launch_range_candidates_lists_bf16x3_as<1, 128>(a, q_hi, q_lo, stream)
	                       : launch_range_candidates_lists_bf16x3_as<2, 128>(a, q_hi, q_lo, stream);
}

#endif // VSS_EXACT_RANGE_TU

} // namespace vss
