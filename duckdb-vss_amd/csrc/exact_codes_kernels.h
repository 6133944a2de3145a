// exact_codes_kernels.h — the exact search's BOUND tile on the int8 matrix pipe, over the index's resident 8-bit row codes
// (option exact.codes_i8, score kind 2).
//
//   k_exact_prepare_codes   per query: the constants of the upper bound (exact_codes_bound.h) from the query's own code record
//   k_exact_bounds_i8       pass A: k_exact_scores_v4's persistent 128 x 128 tile with  I = sum cq_i cx_i  on
//                           v_mfma_i32_32x32x32_i8; the tile's "score" is U(I), an upper bound on the pair's engine distance, so
//                           after the selects best_s[q][k - 1] = tau_q, the k-th smallest upper bound of query q: no row of its
//                           top-k is farther than tau_q
//   k_exact_codes_radii     tau_q -> the radius of pass B (+inf where fewer than k rows had a finite bound)
//   k_exact_codes_topk      after pass B — the range search of kind 2 under those radii, which re-scores in the metric every row
//                           whose LOWER bound is at most tau_q —: per query the k smallest (distance, slot) of its matches
//
// Nothing is certified: the upper and the lower bound hold for every pair, so the matches contain the top-k by construction.
//
// Included at the end of exact_kernels.h (ExactArgs, lex_less); the kernels are defined once, in exact_codes.hip.
#pragma once
#include "exact_codes_bound.h"

namespace vss {

struct ExactCodesPrepareArgs {
	int metric;
	uint32_t n; // padded dimension
	uint32_t n_queries;
	const RowCodeMeta *q_meta; // k_encode_rows over the padded query block
	const uint32_t *norm_ext;  // k_norm_extrema
	ExactCodesQuery *qc;
	unsigned long long *e_max; // bit pattern of the largest finite SLACK (range_codes_slack)
};

// what the bound tile reads in the place of the f32 operands
struct ExactCodesView {
	const uint32_t *q_codes;   // n_queries x V dwords
	const ExactCodesQuery *qc; // n_queries
	const uint32_t *row_codes; // slots x V dwords
	const RowCodeMeta *row_meta;
};

struct ExactCodesTopkArgs {
	uint32_t k;
	const unsigned long long *offsets; // n_queries + 1: query q's matches are cells offsets[q] .. offsets[q + 1]
	const int64_t *slots;              // the matches' SLOTS (RangeRescoreArgs::slots)
	const float *dist;
	const int64_t *keys;
	int64_t *out_keys; // n_queries x k, as k_exact_rerank writes them
	float *out_d;
	uint32_t *out_count;
	const uint32_t *query_map = nullptr; // workgroup b answers query query_map[b] from segment query_map[b] (NULL = identity)
};

hipError_t launch_exact_prepare_codes(const ExactCodesPrepareArgs &a, hipStream_t stream);
// one bound launch over e.row_begin .. e.row_end: `grid` persistent workgroups.  ExactArgs: queries, vectors, row_norm2 and
// query_norm2 are not read.  Needs V % 8 == 0.
hipError_t launch_exact_bounds_i8(const ExactArgs &e, const ExactCodesView &c, uint32_t grid, hipStream_t stream);
// query_map: row t of best_s is the running list of query query_map[t] (the filtered search's group order); NULL = identity
hipError_t launch_exact_codes_radii(const float *best_s, uint32_t k, uint32_t n_queries, float *radii, hipStream_t stream,
                                    const uint32_t *query_map = nullptr);
hipError_t launch_exact_codes_topk(const ExactCodesTopkArgs &a, uint32_t n_queries, hipStream_t stream);

#ifdef VSS_EXACT_CODES_TU

typedef int xc_i32x16 __attribute__((ext_vector_type(16)));
typedef int xc_i32x4 __attribute__((ext_vector_type(4)));
typedef float xc_f32x4 __attribute__((ext_vector_type(4))); // an ExactCodesQuery on its way from memory to LDS, in registers

constexpr uint32_t XC_IMAGE_BYTES = 128 * 128;        // one operand of one step: 128 rows x 128 code bytes
constexpr uint32_t XC_BUF_BYTES = 2 * XC_IMAGE_BYTES; // A | B
constexpr uint32_t XC_LDS_BYTES = 2 * XC_BUF_BYTES;

__global__ __launch_bounds__(256) void k_exact_prepare_codes(ExactCodesPrepareArgs a) {
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= a.n_queries)
		return;
	const RowCodeMeta qm = a.q_meta[q];
	a.qc[q] = exact_codes_query(a.metric, a.n, qm);
	const double S = range_codes_slack(a.metric, a.n, qm, __uint_as_float(a.norm_ext[0]));
	if (S < (double)__builtin_inff())
		atomicMax(a.e_max, (unsigned long long)__double_as_longlong(S));
}

// ---------------------------------------------------------------------------------------------------------
// The tile.  Workgroups, tile order, both epilogues, tombstones, the overflow word and the ragged-tile path are
// k_exact_scores_v4's; operands travel as in range_i8_dots<128> (exact_range_codes_kernels.h), restated here so that a
// persistent workgroup's loads run ahead ACROSS tile boundaries:
//   * a K step is 128 code bytes = 128 dimensions = four MFMA blocks of depth 32; an operand image is 128 rows x 128 bytes with
//     no padding, chunk c (16 bytes) of row r at position c ^ (r & 7) — the eight lanes that stage a row write one 128-byte
//     line, and the MFMA side's ds_read_b128 of chunk 2 kb + (lane >> 5) of rows lane & 31 is conflict-free (the range tile's
//     comment has the argument);
//   * two buffers (64 KiB: two workgroups per compute unit), ONE LDS-only barrier per step: the registers loaded during step
//     g - 1 are written to the idle buffer at the top of step g, the loads of step g + 2 go out behind them.  The load cursor
//     runs two steps ahead of the MFMAs through ALL the workgroup's tiles, so the first step of the next tile is on its way
//     under the current tile's last MFMAs — a 768-dimension row is only six steps, a tile's prologue would be a third of it;
//   * a chunk beyond a row's V / 4 (rows of 32, 64 or 96 dimensions, the last partial step) is staged as zeros;
//   * a lane supplies row lane & 31 and the sixteen k of chunk 2 kb + (lane >> 5) on both operands alike.
// Epilogue: C[row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][col = lane & 31].  The records of a lane's two columns, their keys,
// and (threads 0 .. 127) a query's constants and running k-th best are asked for at the top of the tile's last step; a query's
// {sqm, c1, c2, c3} is then read as one 16-byte LDS word.  U = exact_codes_upper: one convert, one multiply, four fma per pair.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_exact_bounds_i8(ExactArgs a, ExactCodesView v) {
	extern __shared__ __attribute__((aligned(16))) unsigned char xc_smem[];
	__shared__ __attribute__((aligned(16))) ExactCodesQuery qc_l2[2][128]; // by the tile's parity, see the epilogue
	__shared__ __attribute__((aligned(16))) float tau_s2[2][128];
	__shared__ __attribute__((aligned(16))) uint32_t tau_i2[2][128];
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int wm = wave >> 1, wn = wave & 1;
	if (a.cand_cnt && __hip_atomic_load(&a.cand_cnt[a.n_queries], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
		return; // (a filtered pass that has overflowed is repeated the plain way by the host; uniform, as in k_exact_scores_v4)
	const uint32_t chunks = a.V / 4u, steps = (chunks + 7u) / 8u; // (V % 8 == 0: the host's choice of this kernel)
	const uint32_t tx = (a.row_end - a.row_begin + 127u) / 128u, ty = (a.n_queries + 127u) / 128u;
	const uint32_t tx8 = tx & ~7u, T = tx * ty, G = gridDim.x, b = blockIdx.x;
	if (b >= T)
		return;
	auto decode = [&](uint32_t t, uint32_t &x, uint32_t &y) { // as k_exact_scores_v3
		if (t < tx8 * ty) {
			const uint32_t r = t >> 3;
			y = r % ty;
			x = (r / ty) * 8u + (t & 7u);
		} else {
			const uint32_t u = t - tx8 * ty, rem = tx - tx8;
			y = u / rem;
			x = tx8 + u % rem;
		}
	};
	const uint32_t N = ((T - b + G - 1u) / G) * steps; // steps of this workgroup, all its tiles in a row

	xc_i32x16 acc[2][2];
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[i][j][e] = 0;

	// ---- the load side: thread -> chunk f of the step's eight, rows rr + 32 p of both operands; rows beyond the edge re-read the last one
	const uint32_t f = (uint32_t)tid & 7u, rr = (uint32_t)tid >> 3;
	const uint32_t st_off = rr * 128u + ((f ^ (rr & 7u)) << 4); // (rows rr + 32 p: the same row & 7)
	const xc_i32x4 *q_src[4], *x_src[4];
	uint32_t item_l = b, step_l = 0; // the load cursor: two steps ahead of the MFMAs, possibly in the next tile already
	auto set_load_item = [&](uint32_t t) {
		uint32_t x, y;
		decode(t, x, y);
		const uint32_t q0 = y * 128u, r0 = a.row_begin + x * 128u;
#pragma unroll
		for (int p = 0; p < 4; ++p) {
			uint32_t qi = q0 + rr + 32u * p, ri = r0 + rr + 32u * p;
			qi = qi < a.n_queries ? qi : a.n_queries - 1u;
			ri = ri < a.row_end ? ri : a.row_end - 1u;
			q_src[p] = reinterpret_cast<const xc_i32x4 *>(v.q_codes + (size_t)qi * a.V);
			x_src[p] = reinterpret_cast<const xc_i32x4 *>(v.row_codes + (size_t)ri * a.V);
		}
	};
	xc_i32x4 qa[4], xb[4];
	auto load_next = [&]() { // the step under the load cursor -> registers (clamped chunk, zeroed afterwards); advances the cursor
		const uint32_t c = step_l * 8u + f, cc = c < chunks ? c : chunks - 1u;
#pragma unroll
		for (int p = 0; p < 4; ++p)
			qa[p] = q_src[p][cc], xb[p] = x_src[p][cc];
		if (c >= chunks) {
#pragma unroll
			for (int p = 0; p < 4; ++p)
				qa[p] = xb[p] = xc_i32x4 {0, 0, 0, 0};
		}
		if (++step_l == steps) {
			step_l = 0;
			item_l += G;
			if (item_l < T)
				set_load_item(item_l);
		}
	};
	auto store_step = [&](int buf) {
		unsigned char *A = xc_smem + buf * XC_BUF_BYTES + st_off;
#pragma unroll
		for (int p = 0; p < 4; ++p) {
			*reinterpret_cast<xc_i32x4 *>(A + p * 32 * 128) = qa[p];
			*reinterpret_cast<xc_i32x4 *>(A + XC_IMAGE_BYTES + p * 32 * 128) = xb[p];
		}
	};
	// ---- the MFMA side: row lane & 31 of each 32-row tile, chunk 2 kb + (lane >> 5) of block kb, at its swizzled position
	const uint32_t a_row = (uint32_t)(wm * 64 + (lane & 31)) * 128u, b_row = XC_IMAGE_BYTES + (uint32_t)(wn * 64 + (lane & 31)) * 128u;
	uint32_t pos[4];
#pragma unroll
	for (int kb = 0; kb < 4; ++kb)
		pos[kb] = (((uint32_t)(2 * kb) + ((uint32_t)lane >> 5)) ^ ((uint32_t)lane & 7u)) << 4;
	auto read_block = [&](int buf, int kb, xc_i32x4 (&av)[2], xc_i32x4 (&bv)[2]) {
		const unsigned char *I = xc_smem + buf * XC_BUF_BYTES + pos[kb];
#pragma unroll
		for (int i = 0; i < 2; ++i)
			av[i] = *reinterpret_cast<const xc_i32x4 *>(I + a_row + i * 32 * 128);
#pragma unroll
		for (int j = 0; j < 2; ++j)
			bv[j] = *reinterpret_cast<const xc_i32x4 *>(I + b_row + j * 32 * 128);
	};
	auto mfma_block = [&](const xc_i32x4 (&av)[2], const xc_i32x4 (&bv)[2]) { // dependent MFMAs are four issues apart
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
				acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[i], bv[j], acc[i][j], 0, 0, 0);
	};

	// prologue: this workgroup's first step into buffer 0, the second on its way
	set_load_item(b);
	load_next();
	store_step(0);
	if (N > 1)
		load_next();
	lds_barrier();
	uint32_t item_c = b, step_c = 0; // the compute cursor
	uint32_t cx = 0, cy = 0;         // (written only in a tile's last step, as everything its epilogue reads from memory)
	int parity = 0;
	xc_f32x4 my_qc = {0.f, 0.f, 0.f, 0.f};
	float my_tau_s = 0.f;
	uint32_t my_tau_i = 0;
	RowCodeMeta col_meta[2];
	int64_t col_key[2];
#pragma unroll
	for (int j = 0; j < 2; ++j)
		col_meta[j] = RowCodeMeta {0.f, 0.f, 0.f, 0}, col_key[j] = FREE_KEY;
	for (uint32_t g = 0; g < N; ++g) {
		const int buf = (int)(g & 1u);
		const bool last = step_c + 1 == steps;
		if (last) {
			decode(item_c, cx, cy);
#pragma unroll
			for (int j = 0; j < 2; ++j) {
				uint32_t col = a.row_begin + cx * 128u + wn * 64 + j * 32 + (lane & 31);
				col = col < a.row_end ? col : a.row_end - 1u;
				col_meta[j] = v.row_meta[col];
				col_key[j] = a.keys[col];
			}
			if (tid < 128) {
				const uint32_t qi = cy * 128u + tid < a.n_queries ? cy * 128u + tid : a.n_queries - 1u;
				my_qc = reinterpret_cast<const xc_f32x4 *>(v.qc)[qi];
				if (a.cand_cnt) {
					my_tau_s = a.best_s[(size_t)qi * a.KP + a.KP - 1];
					my_tau_i = a.best_i[(size_t)qi * a.KP + a.KP - 1];
				}
			}
		}
		xc_i32x4 av0[2], bv0[2], av1[2], bv1[2];
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
		if (!last) {
			lds_barrier();
			++step_c;
			continue;
		}
		// ---- epilogue of tile (cx, cy).  The step's barrier comes after the constants are in LDS: one barrier serves both.  A
		// row of one step has its next tile's barrier right here, while a slower wave may still read this tile's constants: they
		// alternate between two copies, and a copy is written again only behind the barrier of the tile in between
		ExactCodesQuery *qc_l = qc_l2[parity];
		float *tau_s = tau_s2[parity];
		uint32_t *tau_i = tau_i2[parity];
		parity ^= 1;
		if (tid < 128) {
			reinterpret_cast<xc_f32x4 *>(qc_l)[tid] = my_qc;
			tau_s[tid] = my_tau_s, tau_i[tid] = my_tau_i;
		}
		lds_barrier();
		const uint32_t q0 = cy * 128u, r0 = a.row_begin + cx * 128u;
		const bool whole = q0 + 128u <= a.n_queries && r0 + 128u <= a.row_end;
		auto run = [&](auto mt, auto wh) {
			constexpr int MT = decltype(mt)::value;
			constexpr bool WHOLE = decltype(wh)::value; // every query of the tile exists, every column is a row of the launch
#pragma unroll
			for (int j = 0; j < 2; ++j) {
				const uint32_t col = r0 + wn * 64 + j * 32 + (lane & 31);
				if (!WHOLE && col >= a.row_end)
					continue;
				const ExactCodesRow row = exact_codes_row(MT, a.V * 4u, col_meta[j]);
				const bool dead = col_key[j] == FREE_KEY;
#pragma unroll
				for (int i = 0; i < 2; ++i) {
#pragma unroll
					for (int e4 = 0; e4 < 4; ++e4) {
						const uint32_t ql = wm * 64 + i * 32 + 8 * e4 + 4 * ((uint32_t)lane >> 5);
						float sc[4];
#pragma unroll
						for (int u = 0; u < 4; ++u)
							sc[u] = dead ? __builtin_inff() : exact_codes_upper(acc[i][j][4 * e4 + u], qc_l[ql + u], row);
						if (a.cand_cnt) {
							const float4 ts = *reinterpret_cast<const float4 *>(&tau_s[ql]);
							const uint4 ti = *reinterpret_cast<const uint4 *>(&tau_i[ql]);
							const bool keep[4] = {sc[0] < 3.0e38f && lex_less(sc[0], col, ts.x, ti.x), sc[1] < 3.0e38f && lex_less(sc[1], col, ts.y, ti.y),
							                      sc[2] < 3.0e38f && lex_less(sc[2], col, ts.z, ti.z), sc[3] < 3.0e38f && lex_less(sc[3], col, ts.w, ti.w)};
							if (keep[0] | keep[1] | keep[2] | keep[3]) { // survivors are rare: a few dozen per query and launch
#pragma unroll
								for (int u = 0; u < 4; ++u) {
									const uint32_t qi = q0 + ql + u;
									if (keep[u] && (WHOLE || qi < a.n_queries)) {
										const uint32_t p = atomicAdd(&a.cand_cnt[qi], 1u);
										if (p < a.cand_cap) {
											a.cand_s[(size_t)qi * a.cand_cap + p] = sc[u];
											a.cand_i[(size_t)qi * a.cand_cap + p] = col;
										}
									}
								}
							}
						} else {
#pragma unroll
							for (int u = 0; u < 4; ++u) {
								const uint32_t qi = q0 + ql + u;
								if (WHOLE || qi < a.n_queries)
									a.scores[(size_t)qi * a.chunk_stride + (col - a.row_begin)] = sc[u];
							}
						}
					}
				}
			}
		};
		auto run_metric = [&](auto mt) {
			if (whole)
				run(mt, std::true_type {});
			else
				run(mt, std::false_type {});
		};
		if (a.metric == 0)
			run_metric(std::integral_constant<int, 0> {});
		else if (a.metric == 2)
			run_metric(std::integral_constant<int, 2> {});
		else
			run_metric(std::integral_constant<int, 1> {});
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
#pragma unroll
				for (int e = 0; e < 16; ++e)
					acc[i][j][e] = 0;
		item_c += G;
		step_c = 0;
	}
}

// tau_q -> the radius of pass B.  A k-th best that was never written (the memset's 3.39e38) or is +inf: fewer than k rows had a
// finite bound, and every live row has to be looked at
__global__ __launch_bounds__(256) void k_exact_codes_radii(const float *best_s, uint32_t k, uint32_t n_queries, float *radii,
                                                           const uint32_t *query_map) {
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= n_queries)
		return;
	const float tau = best_s[(size_t)q * k + k - 1];
	radii[query_map ? query_map[q] : q] = tau < 3.0e38f ? tau : __builtin_inff();
}

// ---------------------------------------------------------------------------------------------------------
// The top k of a query's matches by (distance, slot): one workgroup per query, rank by counting.  Thread t holds match
// i = base + t and counts the matches that come before it; the matches it is compared with are staged in LDS, XC_TOPK_LDS
// (distance, slot) pairs at a time and read as broadcasts.  A segment of at most XC_TOPK_LDS matches — the common case by far:
// the match capacity of the call is max(1024, 4 k) cells per query on average — is staged once; a longer one (a query without a
// bound beside others with few matches) is staged again for every 256 matches: quadratic, and still the contract's answer.
// Slots are distinct within a segment, so ranks are too.
constexpr uint32_t XC_TOPK_LDS = 1024;

__global__ __launch_bounds__(256) void k_exact_codes_topk(ExactCodesTopkArgs a) {
	__shared__ float sd[XC_TOPK_LDS];
	__shared__ uint32_t ss[XC_TOPK_LDS];
	const uint32_t q = a.query_map ? a.query_map[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
	const unsigned long long lo = a.offsets[q], n = a.offsets[q + 1] - lo;
	const uint32_t count = n < a.k ? (uint32_t)n : a.k;
	const int64_t *slots = a.slots + lo;
	const float *dist = a.dist + lo;
	for (unsigned long long bi = 0; bi < n; bi += 256) { // (uniform bounds: the barriers below are met by every thread)
		const unsigned long long i = bi + tid;
		const float di = i < n ? dist[i] : 0.f;
		const uint32_t si = i < n ? (uint32_t)slots[i] : 0u;
		uint32_t rank = 0;
		for (unsigned long long bj = 0; bj < n; bj += XC_TOPK_LDS) {
			const uint32_t m = n - bj < XC_TOPK_LDS ? (uint32_t)(n - bj) : XC_TOPK_LDS;
			if (bi == 0 || n > XC_TOPK_LDS) {
				__syncthreads();
				for (uint32_t j = tid; j < m; j += 256)
					sd[j] = dist[bj + j], ss[j] = (uint32_t)slots[bj + j];
				__syncthreads();
			}
			for (uint32_t j = 0; j < m; ++j)
				rank += lex_less(sd[j], ss[j], di, si);
		}
		if (i < n && rank < count) {
			a.out_keys[(size_t)q * a.k + rank] = a.keys[si];
			if (a.out_d)
				a.out_d[(size_t)q * a.k + rank] = di;
		}
	}
	for (uint32_t i = count + tid; i < a.k; i += 256) { // padded as k_exact_rerank pads
		a.out_keys[(size_t)q * a.k + i] = -1ll;
		if (a.out_d)
			a.out_d[(size_t)q * a.k + i] = __builtin_inff();
	}
	if (tid == 0)
		a.out_count[q] = count;
}

// ---------------------------------------------------------------------------------------------------------
hipError_t launch_exact_prepare_codes(const ExactCodesPrepareArgs &a, hipStream_t stream) {
	hipLaunchKernelGGL(k_exact_prepare_codes, dim3((a.n_queries + 255u) / 256u), dim3(256), 0, stream, a);
	return hipGetLastError();
}
hipError_t launch_exact_bounds_i8(const ExactArgs &e, const ExactCodesView &c, uint32_t grid, hipStream_t stream) {
	const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(k_exact_bounds_i8), hipFuncAttributeMaxDynamicSharedMemorySize,
	                                          (int)XC_LDS_BYTES);
	if (rc != hipSuccess)
		return rc;
	hipLaunchKernelGGL(k_exact_bounds_i8, dim3(grid), dim3(256), XC_LDS_BYTES, stream, e, c);
	return hipGetLastError();
}
hipError_t launch_exact_codes_radii(const float *best_s, uint32_t k, uint32_t n_queries, float *radii, hipStream_t stream,
                                    const uint32_t *query_map) {
	hipLaunchKernelGGL(k_exact_codes_radii, dim3((n_queries + 255u) / 256u), dim3(256), 0, stream, best_s, k, n_queries, radii, query_map);
	return hipGetLastError();
}
hipError_t launch_exact_codes_topk(const ExactCodesTopkArgs &a, uint32_t n_queries, hipStream_t stream) {
	hipLaunchKernelGGL(k_exact_codes_topk, dim3(n_queries), dim3(256), 0, stream, a);
	return hipGetLastError();
}

#endif // VSS_EXACT_CODES_TU

} // namespace vss
