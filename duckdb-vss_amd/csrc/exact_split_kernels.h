// exact_split_kernels.h — the exact search's score tile on the bf16 matrix pipe (option exact.split_bf16).
//
//   k_split_queries         the padded query block, once per call, as two bf16 arrays: hi = bf16(q), lo = bf16(q - hi)
//   k_exact_scores_bf16x3   k_exact_scores_v4's persistent 128 x 128 tile with  q.x ~ sum qh xh + qh xl + ql xh  on
//                           v_mfma_f32_32x32x16_bf16 — three MFMAs of depth 16 into one f32 accumulator where the f32 tile
//                           issues eight of depth 2.  The score only SELECTS rows; exact_certificate.h carries the error
//                           bound of this sum (exact_cert_error_split), so every answer stays the contract's.
//
// Included at the end of exact_kernels.h (ExactArgs, exact_score, lex_less, f32x16).  The kernels are defined once, in
// exact_split.hip — a translation unit of its own because it is built without packed f32 arithmetic (the remainders x - hi are
// single v_sub_f32), which must not touch the code of the engine's other kernels; the engine calls the two launchers.
#pragma once
#include "split_bf16.h"

namespace vss {

constexpr uint32_t XS_IMAGE_BYTES = 128 * 64;         // one bf16 image of one operand and step
constexpr uint32_t XS_BUF_BYTES = 4 * XS_IMAGE_BYTES; // A hi | A lo | B hi | B lo
constexpr uint32_t XS_LDS_BYTES = 2 * XS_BUF_BYTES;

// n8 cells of eight floats of the padded query block -> q_hi / q_lo (16 bytes per cell each)
hipError_t launch_split_queries(const float4 *queries, uint64_t n8, uint4 *q_hi, uint4 *q_lo, hipStream_t stream);
// one score launch over e.row_begin .. e.row_end: `grid` persistent workgroups (two per compute unit, at most one per tile)
hipError_t launch_exact_scores_bf16x3(const ExactArgs &e, const uint4 *q_hi, const uint4 *q_lo, uint32_t grid, hipStream_t stream);

// The inline device helpers, for this tile's translation unit and for the range search's (exact_range_split_kernels.h: both are
// built without packed f32 arithmetic).
#if defined(VSS_EXACT_SPLIT_TU) || defined(VSS_EXACT_RANGE_TU)
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4))); // a 16-byte chunk that travels as it is

// two floats -> their bf16 halves: v_cvt_pk_bf16_f32 (round to nearest even), the exact f32 remainders, the convert again.
// Same bits as split_bf16 (split_bf16.h) for finite normal inputs.
__device__ __forceinline__ void split_pair(float a, float b, uint32_t &hi, uint32_t &lo) {
	const f32x2_t v = {a, b};
	hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
	const f32x2_t r = {a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xFFFF0000u)};
	lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2_t));
}
// eight consecutive floats -> one 16-byte chunk of the hi image and one of the lo image
__device__ __forceinline__ void split_chunk(const float4 x0, const float4 x1, uint4 &hi, uint4 &lo) {
	split_pair(x0.x, x0.y, hi.x, lo.x);
	split_pair(x0.z, x0.w, hi.y, lo.y);
	split_pair(x1.x, x1.y, hi.z, lo.z);
	split_pair(x1.z, x1.w, hi.w, lo.w);
}
// where chunk c of row r sits in a bf16 image of 64-byte rows: position c ^ xs_swizzle(r) (the tile's comment below says why)
__device__ __forceinline__ uint32_t xs_swizzle(uint32_t row) {
	return (((row >> 1) ^ (row >> 3)) & 1u) | ((row >> 1) & 2u);
}
#endif

#ifdef VSS_EXACT_SPLIT_TU

// n8 groups of eight floats (the zero-padded query block: n_queries x 4 V floats, V even) -> hi / lo, 16 bytes per group each
__global__ __launch_bounds__(256) void k_split_queries(const float4 *q, uint64_t n8, uint4 *hi, uint4 *lo) {
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (uint64_t)gridDim.x * blockDim.x) {
		uint4 h, l;
		split_chunk(q[2 * i], q[2 * i + 1], h, l);
		hi[i] = h, lo[i] = l;
	}
}

// ---------------------------------------------------------------------------------------------------------
// The tile.  Workgroups, tile order, accumulator layout, ranking scores, both epilogues, tombstones, the overflow word and the
// ragged-tile path are k_exact_scores_v4's; what differs is how operands travel and what the matrix pipe is given.
//   * A step is still 32 floats of K (a 128-byte line of a row) = two MFMA blocks of depth 16.  Its LDS image holds bf16: per
//     operand a hi image and a lo image of 128 rows x 64 bytes, so a step occupies what v4's f32 image does (32 KiB, two
//     buffers).  A row's four 16-byte chunks (eight bf16 each) sit at position  chunk ^ f(row),
//     f(r) = ((r >> 1 ^ r >> 3) & 1) | (r >> 1 & 2):  a row is 64 bytes, so 8 consecutive rows cover the 32 banks twice and 16
//     rows the 64 banks four times; f spreads rows of equal (r & 1) — and of equal (r & 3) — over the four positions, which
//     makes the MFMA operand read (ds_read_b128, 32 consecutive rows at one chunk) and the staging write (ds_write_b128, 4
//     chunks of consecutive rows) conflict-free whether the LDS serves 8 or 16 lanes a cycle.
//   * Rows (operand B) are converted ONCE, on the way into LDS: a thread loads 32 bytes (eight floats = chunk tid & 3 of rows
//     tid >> 2 and + 64) with two global_load_dwordx4, splits them (3 VALU per float) and writes one chunk of each image.  The
//     DMA of v4 cannot convert, so rows are staged through registers as in k_exact_scores_v3, two steps ahead: the loads of
//     step g + 2 are issued during step g, converted and written to the idle buffer during step g + 1.
//   * Queries (operand A) arrive split already (k_split_queries): four 16-byte loads per thread and step, written as they are.
//   * Per block of depth 16 and accumulator: hi.hi, hi.lo, lo.hi — always in this order, term-major over the 2 x 2
//     accumulators so that dependent MFMAs are four issues apart.  A lane supplies row lane & 31 and the eight k of chunk
//     2 kb + (lane >> 5) for both operands (which k a half-wave supplies is free as long as A and B agree).
//   * One LDS barrier per step, placed before the step's second block: the first operands of the next step are read right
//     behind it, under those MFMAs.
// Needs V % 8 == 0 (whole steps), as v4.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void
k_exact_scores_bf16x3(ExactArgs a, const uint4 *q_hi, const uint4 *q_lo) {
	constexpr int TN = 2;
	extern __shared__ __attribute__((aligned(16))) unsigned char x2_smem[];
	__shared__ __attribute__((aligned(16))) float tau_s[128];
	__shared__ __attribute__((aligned(16))) uint32_t tau_i[128];
	const int tid = threadIdx.x;
	const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int wm = wave >> 1, wn = wave & 1;
	if (a.cand_cnt && __hip_atomic_load(&a.cand_cnt[a.n_queries], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
		return; // (a filtered pass that has overflowed is repeated the plain way by the host; uniform: only k_exact_select, stream-ordered against this launch, writes the word)
	const uint32_t steps = a.V / 8; // (V % 8 == 0: the host's choice of this kernel)
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

	f32x16 acc[2][TN];
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < TN; ++j)
#pragma unroll
			for (int e = 0; e < 16; ++e)
				acc[i][j][e] = 0.f;

	// ---- the load side: thread -> chunk c of rows rr and rr + 64 of both operands; rows beyond the edge re-read the last one
	const uint32_t c = (uint32_t)tid & 3u, rr = (uint32_t)tid >> 2;
	const uint32_t st_off = rr * 64u + ((c ^ xs_swizzle(rr)) * 16u); // (row + 64 has the same swizzle: + 64 * 64 bytes)
	const u32x4_t *qh_src[2], *ql_src[2];
	const float4 *x_src[2];
	uint32_t item_l = b, step_l = 0; // the load cursor: two steps ahead of the MFMAs, possibly in the next tile already
	auto set_load_item = [&](uint32_t t) {
		uint32_t x, y;
		decode(t, x, y);
		const uint32_t q0 = y * 128u, r0 = a.row_begin + x * 128u;
#pragma unroll
		for (int p = 0; p < 2; ++p) {
			uint32_t qi = q0 + rr + 64 * p;
			qi = qi < a.n_queries ? qi : a.n_queries - 1;
			qh_src[p] = reinterpret_cast<const u32x4_t *>(q_hi) + (size_t)qi * (a.V / 2) + c; // (a query is V / 2 chunks of eight bf16 in each array)
			ql_src[p] = reinterpret_cast<const u32x4_t *>(q_lo) + (size_t)qi * (a.V / 2) + c;
			uint32_t ri = r0 + rr + 64 * p;
			ri = ri < a.row_end ? ri : a.row_end - 1;
			x_src[p] = a.vectors + (size_t)ri * a.V + 2 * c;
		}
	};
	u32x4_t qh[2], ql[2];
	float4 xb0[2], xb1[2]; // (the two halves of a row's 32 bytes)
	auto load_next = [&]() { // the step under the load cursor -> registers; advances the cursor
#pragma unroll
		for (int p = 0; p < 2; ++p) {
			qh[p] = qh_src[p][step_l * 4];
			ql[p] = ql_src[p][step_l * 4];
			xb0[p] = x_src[p][step_l * 8];
			xb1[p] = x_src[p][step_l * 8 + 1];
		}
		if (++step_l == steps) {
			step_l = 0;
			item_l += G;
			if (item_l < T)
				set_load_item(item_l);
		}
	};
	auto store_step = [&](int buf) { // the registers -> LDS buffer `buf`; the rows are split here, once per element
		unsigned char *A = x2_smem + buf * XS_BUF_BYTES + st_off;
#pragma unroll
		for (int p = 0; p < 2; ++p) {
			uint4 h, l;
			split_chunk(xb0[p], xb1[p], h, l);
			*reinterpret_cast<u32x4_t *>(A + p * 4096) = qh[p];
			*reinterpret_cast<u32x4_t *>(A + XS_IMAGE_BYTES + p * 4096) = ql[p];
			*reinterpret_cast<uint4 *>(A + 2 * XS_IMAGE_BYTES + p * 4096) = h;
			*reinterpret_cast<uint4 *>(A + 3 * XS_IMAGE_BYTES + p * 4096) = l;
		}
	};
	// ---- the MFMA side: row (lane & 31) of each 32-row tile, chunk 2 kb + (lane >> 5) of block kb, at its swizzled position
	const uint32_t a_row = (uint32_t)(wm * 64 + (lane & 31)) * 64u, b_row = 2 * XS_IMAGE_BYTES + (uint32_t)(wn * 32 * TN + (lane & 31)) * 64u;
	uint32_t pos[2];
#pragma unroll
	for (int kb = 0; kb < 2; ++kb)
		pos[kb] = (((uint32_t)(2 * kb) + ((uint32_t)lane >> 5)) ^ xs_swizzle((uint32_t)lane & 31u)) * 16u;
	struct Operands {
		uint4 ah[2], al[2], bh[TN], bl[TN];
	};
	auto read_block = [&](int buf, int kb, Operands &o) {
		const unsigned char *B = x2_smem + buf * XS_BUF_BYTES + pos[kb];
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			o.ah[i] = *reinterpret_cast<const uint4 *>(B + a_row + i * 32 * 64);
			o.al[i] = *reinterpret_cast<const uint4 *>(B + XS_IMAGE_BYTES + a_row + i * 32 * 64);
		}
#pragma unroll
		for (int j = 0; j < TN; ++j) {
			o.bh[j] = *reinterpret_cast<const uint4 *>(B + b_row + j * 32 * 64);
			o.bl[j] = *reinterpret_cast<const uint4 *>(B + XS_IMAGE_BYTES + b_row + j * 32 * 64);
		}
	};
	auto mfma = [&](const uint4 &x, const uint4 &y, f32x16 &d) {
		d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, x), __builtin_bit_cast(bf16x8_t, y), d, 0, 0, 0);
	};
	auto mfma_block = [&](const Operands &o) { // hi.hi, hi.lo, lo.hi: the order is fixed
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < TN; ++j)
				mfma(o.ah[i], o.bh[j], acc[i][j]);
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < TN; ++j)
				mfma(o.ah[i], o.bl[j], acc[i][j]);
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < TN; ++j)
				mfma(o.al[i], o.bh[j], acc[i][j]);
	};

	// prologue: this workgroup's first step into buffer 0, the second on its way
	set_load_item(b);
	load_next();
	store_step(0);
	if (N > 1)
		load_next();
	__syncthreads();
	Operands o0, o1;
	read_block(0, 0, o0);
	uint32_t item_c = b, step_c = 0; // the compute cursor
	uint32_t cx = 0, cy = 0;         // (written only in a tile's last step, as everything its epilogue reads from memory: see v3)
	float my_tau_s = 0.f;
	uint32_t my_tau_i = 0;
	float col_n2[TN];
	int64_t col_key[TN];
#pragma unroll
	for (int j = 0; j < TN; ++j)
		col_n2[j] = 0.f, col_key[j] = FREE_KEY;
	for (uint32_t g = 0; g < N; ++g) {
		const int buf = (int)(g & 1u);
		const bool last = step_c + 1 == steps;
		if (last) {
			decode(item_c, cx, cy);
#pragma unroll
			for (int j = 0; j < TN; ++j) {
				uint32_t col = a.row_begin + cx * 128u + wn * 32 * TN + j * 32 + (lane & 31);
				col = col < a.row_end ? col : a.row_end - 1;
				col_n2[j] = a.row_norm2[col];
				col_key[j] = a.keys[col];
			}
			if (a.cand_cnt && tid < 128) {
				const uint32_t qi = cy * 128u + tid < a.n_queries ? cy * 128u + tid : a.n_queries - 1;
				my_tau_s = a.best_s[(size_t)qi * a.KP + a.KP - 1];
				my_tau_i = a.best_i[(size_t)qi * a.KP + a.KP - 1];
			}
		}
		read_block(buf, 1, o1);
		mfma_block(o0);
		if (g + 1 < N)
			store_step(buf ^ 1); // the registers of the next step (loaded a whole step ago) are split and go to the idle buffer
		if (g + 2 < N && !(a.probe & 2u))
			load_next(); // lands during the next step's MFMAs
		lds_barrier();
		if (g + 1 < N)
			read_block(buf ^ 1, 0, o0);
		mfma_block(o1);
		if (!last || (a.probe & 32u)) {
			if (last)
				item_c += G, step_c = 0;
			else
				++step_c;
			continue;
		}
		// ---- epilogue of tile (cx, cy), as k_exact_scores_v4: C[row = (e&3) + 8*(e>>2) + 4*(lane>>5)][col = lane&31]
		const uint32_t q0 = cy * 128u, r0 = a.row_begin + cx * 128u;
		if (a.cand_cnt) {
			if (tid < 128)
				tau_s[tid] = my_tau_s, tau_i[tid] = my_tau_i;
			lds_barrier();
		}
		const bool whole = q0 + 128u <= a.n_queries && r0 + 128u <= a.row_end && r0 + 128u - a.row_begin <= a.chunk_stride;
		if (whole) {
			// the common case: every query of the tile exists, every column lies inside the window
			const uint32_t qrow = q0 + wm * 64 + 4 * ((uint32_t)lane >> 5); // + 32 i + (e & 3) + 8 (e >> 2)
			auto run = [&](auto mt) {
				constexpr int MT = decltype(mt)::value;
#pragma unroll
				for (int j = 0; j < TN; ++j) {
					const uint32_t col = r0 + wn * 32 * TN + j * 32 + (lane & 31);
					const float xn2 = col_n2[j], rs = MT == 1 ? rsqrtf(col_n2[j]) : 0.f;
					const bool dead = col_key[j] == FREE_KEY;
					if (a.cand_cnt) {
#pragma unroll
						for (int i = 0; i < 2; ++i) {
#pragma unroll
							for (int e4 = 0; e4 < 4; ++e4) {
								const uint32_t ql_ = wm * 64 + i * 32 + 8 * e4 + 4 * ((uint32_t)lane >> 5);
								const float4 ts = *reinterpret_cast<const float4 *>(&tau_s[ql_]);
								const uint4 ti = *reinterpret_cast<const uint4 *>(&tau_i[ql_]);
								float sc[4];
#pragma unroll
								for (int u = 0; u < 4; ++u)
									sc[u] = dead ? __builtin_inff() : exact_score<MT>(acc[i][j][4 * e4 + u], xn2, rs);
								const bool k0 = sc[0] < 3.0e38f && lex_less(sc[0], col, ts.x, ti.x), k1 = sc[1] < 3.0e38f && lex_less(sc[1], col, ts.y, ti.y);
								const bool k2 = sc[2] < 3.0e38f && lex_less(sc[2], col, ts.z, ti.z), k3 = sc[3] < 3.0e38f && lex_less(sc[3], col, ts.w, ti.w);
								if (k0 | k1 | k2 | k3) { // survivors are rare: a few dozen per query and launch
									const bool keep[4] = {k0, k1, k2, k3};
#pragma unroll
									for (int u = 0; u < 4; ++u) {
										if (keep[u]) {
											const uint32_t qi = q0 + ql_ + u;
											const uint32_t p = atomicAdd(&a.cand_cnt[qi], 1u);
											if (p < a.cand_cap) {
												a.cand_s[(size_t)qi * a.cand_cap + p] = sc[u];
												a.cand_i[(size_t)qi * a.cand_cap + p] = col;
											}
										}
									}
								}
							}
						}
					} else if (!(a.probe & 1u)) {
						float *out = a.scores + (size_t)qrow * a.chunk_stride + (col - a.row_begin);
#pragma unroll
						for (int i = 0; i < 2; ++i)
#pragma unroll
							for (int e = 0; e < 16; ++e)
								out[(size_t)(i * 32 + (e & 3) + 8 * (e >> 2)) * a.chunk_stride] =
								    dead ? __builtin_inff() : exact_score<MT>(acc[i][j][e], xn2, rs);
					}
				}
			};
			if (a.metric == 0)
				run(std::integral_constant<int, 0> {});
			else if (a.metric == 2)
				run(std::integral_constant<int, 2> {});
			else
				run(std::integral_constant<int, 1> {});
		} else {
#pragma unroll
			for (int i = 0; i < 2; ++i) {
#pragma unroll
				for (int j = 0; j < TN; ++j) {
					const uint32_t col = r0 + wn * 32 * TN + j * 32 + (lane & 31);
					const bool col_ok = col < a.row_end;
					const float xn2 = col_n2[j];
					const bool live = col_key[j] != FREE_KEY;
#pragma unroll
					for (int e = 0; e < 16; ++e) {
						const uint32_t qi = q0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
						if (qi < a.n_queries && col - a.row_begin < a.chunk_stride) {
							const float dot = acc[i][j][e];
							float s;
							if (a.metric == 0)
								s = xn2 - 2.f * dot;
							else if (a.metric == 2)
								s = -dot;
							else
								s = xn2 > 0.f ? -dot * rsqrtf(xn2) : 0.f;
							if (!col_ok || !live)
								s = __builtin_inff();
							if (a.cand_cnt) {
								const uint32_t ql_ = qi - q0;
								if (s < 3.0e38f && lex_less(s, col, tau_s[ql_], tau_i[ql_])) {
									const uint32_t p = atomicAdd(&a.cand_cnt[qi], 1u);
									if (p < a.cand_cap) {
										a.cand_s[(size_t)qi * a.cand_cap + p] = s;
										a.cand_i[(size_t)qi * a.cand_cap + p] = col;
									}
								}
							} else if (!(a.probe & 1u) || s == 12345.678f)
								a.scores[(size_t)qi * a.chunk_stride + (col - a.row_begin)] = s;
						}
					}
				}
			}
		}
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < TN; ++j)
#pragma unroll
				for (int e = 0; e < 16; ++e)
					acc[i][j][e] = 0.f;
		item_c += G;
		step_c = 0;
	}
}

hipError_t launch_split_queries(const float4 *queries, uint64_t n8, uint4 *q_hi, uint4 *q_lo, hipStream_t stream) {
	const uint32_t grid = (uint32_t)(n8 + 255 < 256ull * 2048 ? (n8 + 255) / 256 : 2048);
	hipLaunchKernelGGL(k_split_queries, dim3(grid), dim3(256), 0, stream, queries, n8, q_hi, q_lo);
	return hipGetLastError();
}
hipError_t launch_exact_scores_bf16x3(const ExactArgs &e, const uint4 *q_hi, const uint4 *q_lo, uint32_t grid, hipStream_t stream) {
	const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(k_exact_scores_bf16x3),
	                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)XS_LDS_BYTES);
	if (rc != hipSuccess)
		return rc;
	hipLaunchKernelGGL(k_exact_scores_bf16x3, dim3(grid), dim3(256), XS_LDS_BYTES, stream, e, q_hi, q_lo);
	return hipGetLastError();
}
#endif // VSS_EXACT_SPLIT_TU

} // namespace vss
